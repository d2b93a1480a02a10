"""Golden vectors of the reference's motion in-painting (diffusion/gaussian_diffusion.py:319-323: y['inpainting_mask'] /
y['inpainted_motion'] inside p_mean_variance), recorded by RUNNING THE REFERENCE (CPU) in the build container.

    python tests/golden/make_golden_inpaint.py [--only NAME]

Same recipe as make_golden.py / make_golden_offline.py (synthetic checkpoints from regennet_amd.synth, noise injected in the reference's
own draw order through _ref_import.NoiseTape). The cases, and the rule that rebuilds each case's mask and target, live in
tests/inpaint_cases.py, shared with the tests; a digest of mask and target is stored beside the result (`inpaint_digest`).
Only DATA is written (tests/golden/inpaint_*.npz).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
from make_golden import build, digest, make_y, save, sd_digest  # noqa: E402
from make_golden_offline import build_offline  # noqa: E402
from regennet_amd import synth  # noqa: E402
from tests.inpaint_cases import CASES, case_inputs  # noqa: E402


def gen(name):
    case, cfg, mask, target = case_inputs(name)
    sd = synth.make_state_dict(cfg, seed=0)
    B, resp, mode, guided = case["B"], case["resp"], case["mode"], case["guided"]
    if cfg.get("arch") == "offline":
        model, diffusion = build_offline(cfg, sd, resp)
    else:
        model, diffusion = build(dict(cfg, noise_schedule="cosine", sigma_small=True), resp, sd)
    S = diffusion.num_timesteps
    y = make_y(cfg, B, guided)
    y["inpainting_mask"] = torch.from_numpy(mask)
    y["inpainted_motion"] = torch.from_numpy(target)
    tape = synth.make_noise_tape(cfg, B, S, seed=10)
    if guided:
        from model.cfg_sampler import ClassifierFreeSampleModel
        fmodel = ClassifierFreeSampleModel(model)
    else:
        fmodel = model
    shape = (B, cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    fn = diffusion.p_sample_loop_progressive if mode == "ddpm" else diffusion.ddim_sample_loop_progressive
    x0s, xs = [], []
    t0 = time.time()
    with _ref_import.NoiseTape(tape) as nt, torch.no_grad():
        for out in fn(fmodel, shape, clip_denoised=bool(case.get("clip", False)), model_kwargs={"y": y}):
            if case.get("trace"):
                x0s.append(out["pred_xstart"].numpy().copy())
                xs.append(out["sample"].numpy().copy())
            final = out["sample"]
        assert nt.pos == S + 1, (nt.pos, S)
    dt = time.time() - t0
    final = final.numpy()
    print(f"{name}: reference {mode} S={S} B={B} took {dt:.1f}s")
    kw = dict(cfg_name=case["cfg_name"], over=repr({}), opts=repr({}), B=B, resp=resp, mode=mode, guided=guided, S=S,
              clip=bool(case.get("clip", False)), ref_seconds=dt, sd_digest=sd_digest(sd),
              in_digest=digest(tape[0], tape[-1], y["cmotion"].numpy()), inpaint_digest=digest(mask, target),
              mask_rule=repr(case["masks"]), target_rule=repr(("make_noise_tape", 12, case.get("target_scale", 0.5))))
    if "rows" in case:
        rows = np.array(case["rows"], dtype=np.int64)
        kw.update(rows=rows, final_rows=final[rows])
    else:
        kw.update(final=final)
    if case.get("trace"):
        kw.update(x0=np.stack(x0s), x=np.stack(xs))
    save(name, **kw)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    torch.set_num_threads(8)
    for k in CASES:
        if a.only is None or a.only == k:
            gen(k)
