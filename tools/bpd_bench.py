"""Time diffusion.calc_bpd_loop against the reference-structured loop:  python tools/bpd_bench.py [--out profiles/bpd_bench.txt]

NTU shape (B = 8 motions of [56, 6, 60], the 8-layer d = 512 model on the synthetic checkpoint), the whole cosine-1000 schedule, on the same GPU
in the same process, the two sides alternating, each figure the median of 3 whole evaluations between device events, warmed up:
  batched    diffusion.calc_bpd_loop(max_rows_per_call=256): 32 timesteps x 8 motions per evaluation - per evaluation one rgn_q_sample_rows
             (noise drawn in the kernel), one forward of 256 rows, one rgn_vb_terms
  per step   the reference's structure (gaussian_diffusion.py:1546-1601) through this project's model: per timestep one randn_like, q_sample, one
             forward of B rows and the terms as torch expressions in fp32 on the device (tests/bpd_ref.py's)
  kernels    the two new kernels alone on the batched path's shapes (32 calls of 256 rows each): their share of the batched time
Nothing here is a pass / fail check."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from regennet_amd import _lib, synth  # noqa: E402
from tests import bpd_ref  # noqa: E402

B, ROWS, REPEATS = 8, 256, 3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def per_step_loop(diffusion, model, x0, y):
    """The reference's loop body per timestep; -> vb [B, S] in its column order."""
    S = diffusion.num_timesteps
    vb = []
    for t in range(S - 1, -1, -1):
        tb = torch.full((x0.shape[0],), t, device=x0.device, dtype=torch.long)
        noise = torch.randn_like(x0)
        x_t = diffusion.q_sample(x0, tb, noise)
        with torch.no_grad():
            out = diffusion.p_mean_variance(model, x_t, tb, clip_denoised=True, model_kwargs={"y": y})
        true_mean, _, true_lv = diffusion.q_posterior_mean_variance(x0, x_t, tb)
        kl = bpd_ref.normal_kl(true_mean, true_lv, out["mean"], out["log_variance"]).flatten(1).mean(1) / math.log(2.0)
        nll = -bpd_ref.discretized_gaussian_log_likelihood(x0, out["mean"], 0.5 * out["log_variance"]).flatten(1).mean(1) / math.log(2.0)
        vb.append(torch.where(tb == 0, nll, kl))
        ((out["pred_xstart"] - x0) ** 2).flatten(1).mean(1)
        ((diffusion._predict_eps_from_xstart(x_t, tb, out["pred_xstart"]) - noise) ** 2).flatten(1).mean(1)
    return torch.stack(vb, 1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--steps", default="", help="timestep respacing (default: the whole 1000-step schedule)")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs a GPU: numbers that were not measured on one are reported as 'not measured'"
    cfg = synth.get_config("ntu")
    model, diffusion = synth.build_model(cfg, synth.make_state_dict(cfg, seed=0), resp=args.steps)
    S = diffusion.num_timesteps
    dev = next(model.parameters()).device
    x0 = torch.from_numpy(synth.make_cmotion(cfg, B, seed=4)).to(dev)
    y = {"cmotion": torch.from_numpy(synth.make_cmotion(cfg, B, seed=1)).to(dev)}
    shape = tuple(x0.shape[1:])

    def batched():
        return diffusion.calc_bpd_loop(model, x0, model_kwargs={"y": y}, seed=1, max_rows_per_call=ROWS)["vb"]

    def per_step():
        return per_step_loop(diffusion, model, x0, y)

    per = ROWS // B
    t_rows = np.repeat(np.arange(per - 1, -1, -1), B)
    t32 = torch.from_numpy(t_rows.astype(np.int32)).to(dev)
    qc, coef = torch.from_numpy(bpd_ref.q_coef_rows(diffusion, t_rows)).to(dev), torch.from_numpy(bpd_ref.coef_rows(diffusion, t_rows)).to(dev)
    x_t, noise, terms = torch.empty((ROWS,) + shape, device=dev), torch.empty((ROWS,) + shape, device=dev), torch.empty((ROWS, 3), device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    calls = -(-S // per)

    def kernels():
        eng = model._engine
        for _ in range(calls):
            eng.q_sample_rows(x0, None, qc, t32, 1, 0, x_t, noise, stream)
            eng.vb_terms(x0, x_t, x_t, noise, t32, coef, _lib.VB_CLIP, terms, stream)

    a, b = batched(), per_step()                       # warm-up; both sides computed the same kind of thing (parity is tests/test_bpd_gpu.py)
    kernels()
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.isfinite(b).all() and a.shape == b.shape == (B, S)
    b_ms, p_ms, k_ms = [], [], []
    for _ in range(REPEATS):
        b_ms.append(timed(batched)[0])
        p_ms.append(timed(per_step)[0])
        k_ms.append(timed(kernels)[0])
    bm, pm, km = statistics.median(b_ms), statistics.median(p_ms), statistics.median(k_ms)
    lines = [f"calc_bpd_loop on {torch.cuda.get_device_name(0)}: B = {B} motions of {list(shape)}, S = {S} timesteps, NTU model ({model.precision}); device events around "
             f"whole evaluations, the sides alternating, median of {REPEATS} (min .. max)",
             f"batched, {ROWS} rows per call ({calls} calls)   {bm:9.1f} ms ({min(b_ms):.1f} .. {max(b_ms):.1f})   {bm / S * 1e3:8.1f} us per timestep",
             f"per step, {B} rows per call ({S} calls)   {pm:9.1f} ms ({min(p_ms):.1f} .. {max(p_ms):.1f})   {pm / S * 1e3:8.1f} us per timestep",
             f"per step / batched                       {pm / bm:9.2f}",
             f"rgn_q_sample_rows + rgn_vb_terms alone   {km:9.2f} ms ({min(k_ms):.2f} .. {max(k_ms):.2f})   {100 * km / bm:5.1f} % of the batched time"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
