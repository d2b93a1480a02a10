"""Same-box A/B: an arch='offline' handle against an online emb_trans_dec handle of the same shapes and plan (both run every step
split-bf16 under the default precision rule for embedding-token models), alternating calls, device-synchronised.

    python tools/offline_ab.py --config ntu --batch 256 --respacing "" --calls 5
    python tools/offline_ab.py --config chi3d --batch 128 --respacing "" --calls 5

Prints one JSON line: per arch the median / min / max seconds per sampling call and motions/s, and the offline / online ratio.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from regennet_amd import synth  # noqa: E402
from tests.helpers import y_to_device  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ntu")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--respacing", default="")
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    B = a.batch
    runs = {}
    for arch, cfg in (("offline", synth.get_config(a.config + "_offline")), ("online_etd", synth.get_config(a.config, emb_trans_dec=True))):
        sd = synth.make_state_dict(cfg, seed=0)
        model, diffusion = synth.build_model(cfg, sd, resp=a.respacing, device="cuda:0")
        y = {"cmotion": synth.make_cmotion(cfg, B, seed=1)}
        if "action" in cfg["cond_mode"]:
            y["action"] = synth.make_actions(cfg, B, seed=2)
        shape = (B, cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
        runs[arch] = (model, diffusion, y_to_device(y), shape)
    times = {k: [] for k in runs}

    def call(arch, seed):
        model, diffusion, y, shape = runs[arch]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = diffusion.p_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": y}, seed=seed)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        return time.perf_counter() - t0

    for arch in runs:                       # warm-up: engine build, graph capture
        call(arch, 1)
    for i in range(a.calls):
        for arch in (("offline", "online_etd") if i % 2 == 0 else ("online_etd", "offline")):
            times[arch].append(call(arch, 100 + i))
    plan = {k: {c: v["kernel"] for c, v in runs[k][0]._engine.plan_query(B, split_phase=True).items()} for k in runs}
    res = {k: dict(median_s=statistics.median(v), min_s=min(v), max_s=max(v), motions_per_s=B / statistics.median(v), plan_split_phase=plan[k])
           for k, v in times.items()}
    print(json.dumps(dict(config=a.config, batch=B, respacing=a.respacing or "1000-step DDPM", calls=a.calls, results=res,
                          offline_over_online_etd=res["offline"]["median_s"] / res["online_etd"]["median_s"])))


if __name__ == "__main__":
    main()
