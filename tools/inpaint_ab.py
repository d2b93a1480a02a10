"""Same-box A/B of motion in-painting: one model, alternating calls, device-synchronised. Three arms:

    plain      the fused loop without a mask
    fused      the fused loop with an in-between mask (rgn_set_inpainting: the INPAINT forms of the step boundary)
    per_step   the same mask through _loop_per_step (one rgn_denoise per step + torch glue): the path these calls took before

    python tools/inpaint_ab.py --config ntu --batch 256 --respacing "" --calls 5
    python tools/inpaint_ab.py --config ntu_action --batch 64 --respacing ddim100 --guided --calls 7 --loops 10
    python tools/inpaint_ab.py --config ntu_action --batch 64 --respacing ddim100 --guided --layers_guided 2 --calls 7 --loops 10
    python tools/inpaint_ab.py --config ntu_action --batch 256 --respacing ddim100 --guided --calls 7 --loops 4

(the first guided line runs k_layers<false> + the guided k_step per step - the default at 2 B <= #CUs; --layers_guided 2, or B = 256, runs the
guided k_layers<true> form, a motion per workgroup.) Every arm is warmed up; a timed call is --loops sampling calls back to back, so that a
short loop still gives a window of a good fraction of a second. Appends one JSON line to profiles/inpaint_ab.jsonl (and prints it): per arm
the median / min / max seconds per sampling call and motions/s, and the ratios fused / plain and per_step / fused. --per_step_calls sets the
slow arm's count (default 3). --only ARM runs that arm alone and writes nothing: the form to put under a kernel trace.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from regennet_amd import synth  # noqa: E402
from regennet_amd.sample.edit import in_between_mask  # noqa: E402
from tests.helpers import y_to_device  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ntu")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--respacing", default="")
    ap.add_argument("--guided", action="store_true")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--per_step_calls", type=int, default=3)
    ap.add_argument("--loops", type=int, default=1, help="sampling calls per timed window")
    ap.add_argument("--layers_guided", type=int, default=None, help="engine option LAYERS_GUIDED (0 | 1 | 2)")
    ap.add_argument("--only", default=None, choices=["plain", "fused", "per_step"])
    a = ap.parse_args()
    B = a.batch
    cfg = synth.get_config(a.config)
    sd = synth.make_state_dict(cfg, seed=0)
    opts = None if a.layers_guided is None else {"LAYERS_GUIDED": a.layers_guided}
    model, diffusion = synth.build_model(cfg, sd, resp=a.respacing, device="cuda:0", engine_options=opts)
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=1)}
    if "action" in cfg["cond_mode"]:
        y["action"] = synth.make_actions(cfg, B, seed=2)
    y = y_to_device(y)
    fm = model
    if a.guided:
        from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
        fm = ClassifierFreeSampleModel(model)
        y["scale"] = torch.full((B,), 2.5, device="cuda:0")
    shape = (B, cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    yi = dict(y, inpainting_mask=torch.from_numpy(in_between_mask(shape, 0.25, 0.75)).cuda(),
              inpainted_motion=torch.from_numpy(synth.make_cmotion(cfg, B, seed=4)).cuda())
    fn = diffusion.ddim_sample_loop if a.respacing.startswith("ddim") else diffusion.p_sample_loop
    arms = {"plain": (y, {}), "fused": (yi, {}), "per_step": (yi, {"_per_step": True})}
    times = {k: [] for k in arms}

    def call(arm, seed, loops=None):
        yy, kw = arms[arm]
        loops = a.loops if loops is None else loops
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(loops):
            out = fn(fm, shape, clip_denoised=False, model_kwargs={"y": yy}, seed=seed + 1000 * k, **kw)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / loops
        assert torch.isfinite(out).all()
        return dt

    if a.only:
        call(a.only, 1, 1)
        print(json.dumps({a.only: [call(a.only, 100 + i) for i in range(a.calls)]}))
        return
    for arm in arms:                             # warm-up: engine build, calibration, graph capture, the per-step path's engine state
        call(arm, 1, 1)
    for i in range(a.calls):
        for arm in (("plain", "fused") if i % 2 == 0 else ("fused", "plain")):
            times[arm].append(call(arm, 100 + i))
    for i in range(a.per_step_calls):
        times["per_step"].append(call("per_step", 100 + i, 1))
    res = {k: dict(median_s=statistics.median(v), min_s=min(v), max_s=max(v), motions_per_s=B / statistics.median(v), calls=len(v))
           for k, v in times.items() if v}
    plan = {c: v["kernel"] for c, v in model._engine.plan_query(B, guided=a.guided, split_phase=False).items()}
    line = dict(config=a.config, batch=B, respacing=a.respacing or "1000-step DDPM", guided=a.guided, layers_guided=a.layers_guided, loops=a.loops,
                device=torch.cuda.get_device_name(0), plan_plain_phase=plan,
                results=res, fused_over_plain=res["fused"]["median_s"] / res["plain"]["median_s"])
    if "per_step" in res:
        line["per_step_over_fused"] = res["per_step"]["median_s"] / res["fused"]["median_s"]
    text = json.dumps(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "inpaint_ab.jsonl"), "a") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
