"""Golden vectors of the reference's arch='offline' denoiser, recorded by RUNNING THE REFERENCE (CPU) in the build container.

    python tests/golden/make_golden_offline.py [--only NAME]

The offline model is the non-causal `nn.TransformerEncoder` branch of the reference's `CMDM.forward` (model/cmdm.py:228-238).
Same recipe as make_golden.py (synthetic checkpoints from regennet_amd.synth with the reference's key names, noise injected in
the reference's own draw order through _ref_import.NoiseTape), with the reference CMDM constructed here with arch='offline'.
Only DATA is written (tests/golden/offline_*.npz, offline_keys.json).
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
from make_golden import digest, make_y, save, sd_digest  # noqa: E402
from regennet_amd import synth  # noqa: E402


def build_offline(cfg, sd, resp=""):
    """The reference CMDM(arch='offline') + SpacedDiffusion for a synth config and checkpoint."""
    _ref_import.install()
    from diffusion import gaussian_diffusion as gd
    from diffusion.respace import SpacedDiffusion, space_timesteps
    from model.cmdm import CMDM

    assert cfg["arch"] == "offline"
    with contextlib.redirect_stdout(io.StringIO()):
        model = CMDM("", cfg["njoints"], cfg["nfeats"], cfg["num_actions"], True, "rot6d", True, True,
                     num_frames=cfg["num_frames"], latent_dim=cfg["latent_dim"], ff_size=cfg["ff_size"],
                     num_layers=cfg["layers"], num_heads=cfg["num_heads"], dropout=0.1, activation="gelu",
                     data_rep="rot6d", dataset=cfg["dataset"], arch="offline", cm_mode=cfg["cm_mode"],
                     body_model="smplx", cond_mode=cfg["cond_mode"], cond_mask_prob=cfg["cond_mask_prob"],
                     action_emb="tensor", emb_trans_dec=False, wo_pos_emb=False)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    assert not unexpected, unexpected
    assert all(k.startswith("clip_model.") for k in missing), missing
    model.eval()
    diffusion = SpacedDiffusion(use_timesteps=space_timesteps(1000, resp or [1000]),
                                betas=gd.get_named_beta_schedule("cosine", 1000, 1.0),
                                model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                                loss_type=gd.LossType.MSE, rescale_timesteps=False, data_rep="rot6d", num_person=1,
                                body_model="smplx")
    return model, diffusion


def gen_keys():
    out = {}
    for name in ("tiny_offline", "ntu_offline"):
        cfg = synth.get_config(name)
        model, _ = build_offline(cfg, synth.make_state_dict(cfg, seed=0))
        out[name] = {k: list(v.shape) for k, v in model.state_dict().items() if not k.startswith("clip_model.")}
    path = os.path.join(HERE, "offline_keys.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote", path)


def gen_forward(name, cfg_name, B, ts, guided=False, uncond_ts=()):
    cfg = synth.get_config(cfg_name)
    sd = synth.make_state_dict(cfg, seed=0)
    model, _ = build_offline(cfg, sd)
    y = make_y(cfg, B, guided)
    x = torch.from_numpy(synth.make_noise_tape(cfg, B, 0, seed=11)[0])
    if guided:
        from model.cfg_sampler import ClassifierFreeSampleModel
        fmodel = ClassifierFreeSampleModel(model)
    else:
        fmodel = model
    with torch.no_grad():
        outs = [fmodel(x, torch.tensor([t] * B), y=y).numpy() for t in ts]
        outs_u = [model(x, torch.tensor([t] * B), y=dict(y, uncond=True)).numpy() for t in uncond_ts]
    kw = dict(cfg_name=cfg_name, over=repr({}), B=B, ts=np.array(ts), guided=guided, out=np.stack(outs),
              sd_digest=sd_digest(sd), in_digest=digest(x.numpy(), y["cmotion"].numpy()))
    if uncond_ts:
        kw.update(uncond_ts=np.array(uncond_ts), out_uncond=np.stack(outs_u))
    save(name, **kw)


def gen_loop(name, cfg_name, B, resp, mode, guided=False, keep_trace=False):
    cfg = synth.get_config(cfg_name)
    sd = synth.make_state_dict(cfg, seed=0)
    model, diffusion = build_offline(cfg, sd, resp)
    S = diffusion.num_timesteps
    y = make_y(cfg, B, guided)
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
    with _ref_import.NoiseTape(tape) as nt:
        for out in fn(fmodel, shape, clip_denoised=False, model_kwargs={"y": y}):
            if keep_trace:
                x0s.append(out["pred_xstart"].numpy().copy())
                xs.append(out["sample"].numpy().copy())
            final = out["sample"]
        assert nt.pos == S + 1, (nt.pos, S)
    dt = time.time() - t0
    print(f"{name}: reference {mode} S={S} B={B} took {dt:.1f}s")
    kw = dict(cfg_name=cfg_name, over=repr({}), opts=repr({}), B=B, resp=resp, mode=mode, guided=guided, S=S,
              final=final.numpy(), ref_seconds=dt, sd_digest=sd_digest(sd),
              in_digest=digest(tape[0], tape[-1], y["cmotion"].numpy()))
    if keep_trace:
        kw.update(x0=np.stack(x0s), x=np.stack(xs))
    save(name, **kw)


def gen_loop_rows(name, cfg_name, B, resp, mode, guided, rows):
    """A loop at a batch too large to store whole: only the final samples of `rows` are kept (the rest of the batch still runs,
    so the recorded rows are those of the full-batch call)."""
    cfg = synth.get_config(cfg_name)
    sd = synth.make_state_dict(cfg, seed=0)
    model, diffusion = build_offline(cfg, sd, resp)
    S = diffusion.num_timesteps
    y = make_y(cfg, B, guided)
    tape = synth.make_noise_tape(cfg, B, S, seed=10)
    from model.cfg_sampler import ClassifierFreeSampleModel
    fmodel = ClassifierFreeSampleModel(model) if guided else model
    shape = (B, cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    fn = diffusion.p_sample_loop if mode == "ddpm" else diffusion.ddim_sample_loop
    t0 = time.time()
    with _ref_import.NoiseTape(tape) as nt, torch.no_grad():
        final = fn(fmodel, shape, clip_denoised=False, model_kwargs={"y": y})
        assert nt.pos == S + 1, (nt.pos, S)
    dt = time.time() - t0
    print(f"{name}: reference {mode} S={S} B={B} took {dt:.1f}s")
    rows = np.array(rows, dtype=np.int64)
    save(name, cfg_name=cfg_name, over=repr({}), opts=repr({}), B=B, resp=resp, mode=mode, guided=guided, S=S, rows=rows,
         final_rows=final.numpy()[rows], ref_seconds=dt, sd_digest=sd_digest(sd), in_digest=digest(tape[0], tape[-1], y["cmotion"].numpy()))


def gen_autoreg(name, cfg_name, B, resp):
    """The auto_regressive frame loop of eval/a2m/stgcn_eval.py:50-67 (setting 'cmdm'), restated around the reference's own
    offline model and p_sample_loop as make_golden.gen_autoreg does for the online one: frame f reveals the actor up to f
    (later frames zero), runs a full sampler with tape seed 100 + f and keeps frame f."""
    cfg = synth.get_config(cfg_name)
    sd = synth.make_state_dict(cfg, seed=0)
    model, diffusion = build_offline(cfg, sd, resp)
    S = diffusion.num_timesteps
    y = make_y(cfg, B, False)
    T = cfg["num_frames"]
    shape = (B, cfg["njoints"], cfg["nfeats"], T)
    cmotion_bak = y["cmotion"]
    cmotion = torch.zeros_like(cmotion_bak)
    output = torch.zeros((B, cfg["njoints"], cfg["nfeats"] * 2, T))
    t0 = time.time()
    for f in range(T):
        cmotion[:, :, :, f] = cmotion_bak[:, :, :, f]
        y["cmotion"] = cmotion
        tape = synth.make_noise_tape(cfg, B, S, seed=100 + f)
        with _ref_import.NoiseTape(tape) as nt:
            sample = diffusion.p_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": y})
            assert nt.pos == S + 1
        output[:, :, :, f] = torch.cat((y["cmotion"], sample), axis=2)[:, :, :, f]
    dt = time.time() - t0
    print(f"{name}: reference auto_regressive T={T} S={S} B={B} took {dt:.1f}s")
    save(name, cfg_name=cfg_name, over=repr({}), B=B, resp=resp, S=S, T=T, guided=False, output=output.numpy(), ref_seconds=dt,
         sd_digest=sd_digest(sd), in_digest=digest(synth.make_noise_tape(cfg, B, S, seed=100)[0], cmotion_bak.numpy()))


JOBS = {
    "keys": gen_keys,
    "offline_tiny_fwd": lambda: gen_forward("offline_tiny_fwd", "tiny_offline", 3, [0, 10, 500, 999], uncond_ts=[500]),
    "offline_tiny_fwd_cfg": lambda: gen_forward("offline_tiny_fwd_cfg", "tiny_offline", 3, [10, 700], guided=True),
    "offline_ntu_fwd": lambda: gen_forward("offline_ntu_fwd", "ntu_offline", 2, [10, 999]),
    "offline_chi3d_fwd": lambda: gen_forward("offline_chi3d_fwd", "chi3d_offline", 1, [700], guided=True, uncond_ts=[700]),
    "offline_tiny_add_ddpm10": lambda: gen_loop("offline_tiny_add_ddpm10", "tiny_add_offline", 2, "10", "ddpm", keep_trace=True),
    "offline_tiny_ddim10_cfg": lambda: gen_loop("offline_tiny_ddim10_cfg", "tiny_offline", 2, "ddim10", "ddim", guided=True),
    "offline_ntu_ddpm50": lambda: gen_loop("offline_ntu_ddpm50", "ntu_offline", 2, "50", "ddpm"),
    "offline_chi3d_ddim20_cfg": lambda: gen_loop("offline_chi3d_ddim20_cfg", "chi3d_offline", 1, "ddim20", "ddim", guided=True),
    "offline_ntu_action_ddim5_cfg_b64": lambda: gen_loop_rows("offline_ntu_action_ddim5_cfg_b64", "ntu_action_offline", 64, "ddim5", "ddim",
                                                            True, [0, 1, 21, 42, 63]),
    "offline_tiny_add_autoreg_ddpm10": lambda: gen_autoreg("offline_tiny_add_autoreg_ddpm10", "tiny_add_offline", 2, "10"),
}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    torch.set_num_threads(8)
    for k, fn in JOBS.items():
        if a.only is None or a.only == k:
            fn()
