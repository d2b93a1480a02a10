"""arch='mlp' on one box: the HIP mixer stack against tests/mlp_arch_ref.py run as torch ops on the same GPU, and what the 2 L launches per
evaluation cost.

    python tools/mlp_arch_bench.py --config ntu_mlp --batch 256 --respacing 50 --calls 5

Prints one JSON line:
  hip_ms_per_eval          a sampling step of the engine (captured graphs, default precision schedule): --calls windows of one S-step sampling call
                           each, between device events, alternating with the torch windows; median (min / max beside it)
  hip_kernel_ms_per_eval   per kernel class, the event-bracketed time of one evaluation's launches run one after the other (profiling mode: one
                           chain, no graph), less the bracket's own overhead; "stack" sums the mixer class and the L feature-mix GEMMs' share
  torch_stack_ms           mlp_arch_ref.mixer_stack (fp32 torch ops, the same weights and shapes) on the GPU: --calls windows of S evaluations back to
                           back between device events; median (min / max beside it)
  boundary_share           1 - (sum of the evaluation's kernel times) / (its un-overlapped wall time in profiling mode): the part of an evaluation
                           spent between launches - the case for or against a one-launch stack
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from regennet_amd import synth  # noqa: E402
from tests import mlp_arch_ref  # noqa: E402
from tests.helpers import y_to_device  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ntu_mlp")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--respacing", default="50")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--precision", default="bf16_x3tail")
    a = ap.parse_args()
    B = a.batch
    cfg = synth.get_config(a.config)
    sd = synth.make_state_dict(cfg, seed=0)
    model, diffusion = synth.build_model(cfg, sd, resp=a.respacing, precision=a.precision, device="cuda:0")
    S = diffusion.num_timesteps
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=1)}
    if "action" in cfg["cond_mode"]:
        y["action"] = synth.make_actions(cfg, B, seed=2)
    y = y_to_device(y)
    shape = (B, cfg["njoints"], cfg["nfeats"], cfg["num_frames"])

    def call(seed):
        """One sampling call of S steps between two device events on the caller's stream (the engine joins it by events): ms per call."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = diffusion.p_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": y}, seed=seed)
        e1.record()
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        return e0.elapsed_time(e1)

    L, d, T = cfg["layers"], cfg["latent_dim"], cfg["num_frames"]
    F = cfg["njoints"] * cfg["nfeats"]
    sdc = {k: torch.from_numpy(v).cuda() for k, v in sd.items()}
    h = torch.randn(B, T, d, device="cuda")
    emb = torch.randn(B, d, device="cuda")

    def torch_window(iters):
        """`iters` evaluations of the restatement's stack back to back between two device events: ms per evaluation."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.no_grad():
            e0.record()
            for _ in range(iters):
                out = mlp_arch_ref.mixer_stack(sdc, cfg, h, emb)
            e1.record()
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        return e0.elapsed_time(e1) / iters

    call(1)                                       # warm-up: engine build, graph capture
    torch_window(S)
    hip_w, torch_w = [], []
    for i in range(a.calls):                      # the two sides alternate, windows of S evaluations each (S x 2 ms >> the event resolution)
        hip_w.append(call(100 + i) / S)
        torch_w.append(torch_window(S))
    hip_eval, torch_stack = statistics.median(hip_w), statistics.median(torch_w)
    eng = model._engine
    plan = {c: v for c, v in eng.plan_query(B, split_phase=True).items() if v["launches_per_eval"] > 0}
    # profiling mode: every launch bracketed by events, one chain, no graph
    eng.profile_enable(True)
    wall = call(7) / S
    prof = eng.profile_query()
    bracket = eng.profile_bracket_overhead_ms()
    eng.profile_enable(False)
    per_eval = {c: (ms - n * bracket) / S for c, (ms, n) in prof.items() if n > 0}
    gemm_flops = {"feature_mix": L * d * d * T, "embed_project": 2 * F * d * T, "emb_fc": L * d * d}
    share = gemm_flops["feature_mix"] / sum(gemm_flops.values())
    stack = per_eval.get("mixer", 0.0) + share * per_eval.get("gemm_mfma", 0.0)
    busy = sum(per_eval.values())

    print(json.dumps(dict(config=a.config, batch=B, steps=S, precision=a.precision, device=torch.cuda.get_device_name(0),
                          hip_ms_per_eval=hip_eval, hip_ms_per_eval_min_max=[min(hip_w), max(hip_w)], torch_stack_ms_min_max=[min(torch_w), max(torch_w)], evals_per_window=S, motions_per_s=B / (hip_eval * S / 1e3), hip_profiled_wall_ms_per_eval=wall,
                          hip_kernel_ms_per_eval=dict(per_eval, stack=stack), launches_per_eval={c: v["launches_per_eval"] for c, v in plan.items()},
                          kernels={c: v["kernel"] for c, v in plan.items()}, torch_stack_ms=torch_stack,
                          hip_stack_over_torch=stack / torch_stack, boundary_share=1.0 - busy / wall)))


if __name__ == "__main__":
    main()
