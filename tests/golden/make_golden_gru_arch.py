"""Golden vectors of the reference's arch='gru' denoiser, recorded by RUNNING THE REFERENCE (CPU) in the build container.

    python tests/golden/make_golden_gru_arch.py [--only NAME]

The gru model is the nn.GRU branch of the reference's `CMDM.forward` (model/cmdm.py:191-199, 243-249), cm_mode='add'. Same recipe as
make_golden_mlp.py (synthetic checkpoints from regennet_amd.synth with the reference's key names, noise injected in the reference's own
draw order through _ref_import.NoiseTape), with the reference CMDM constructed here with arch='gru'. The reference hands [T, B, d] to a
batch_first GRU, so its recurrence runs over the samples of a call: that is scan='batch'. For scan='frames' the SAME reference model is
used with its `gru` submodule called on the transposed sequence. The cases live in tests/gru_arch_cases.py, shared with the tests. Every
recorded output must have max-abs in [1, 4]: the synthetic weights are scaled so that the absolute parity bounds of the tests mean
something. Only DATA is written (tests/golden/gru_arch_*.npz, gru_arch_keys.json).
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
from tests.gru_arch_cases import FORWARD, LOOPS, inpaint_inputs  # noqa: E402


class _OverFrames(torch.nn.Module):
    """The reference's own nn.GRU, called on the transposed sequence: the recurrence then runs over the frames of every sample."""

    def __init__(self, gru):
        super().__init__()
        self.inner = gru

    def forward(self, xseq):
        out, h = self.inner(xseq.transpose(0, 1))
        return out.transpose(0, 1), h


def build_gru(cfg, sd, resp="", scan="batch"):
    """The reference CMDM(arch='gru') + SpacedDiffusion for a synth config and checkpoint."""
    _ref_import.install()
    from diffusion import gaussian_diffusion as gd
    from diffusion.respace import SpacedDiffusion, space_timesteps
    from model.cmdm import CMDM

    assert cfg["arch"] == "gru" and cfg["cm_mode"] == "add"
    with contextlib.redirect_stdout(io.StringIO()):
        model = CMDM("", cfg["njoints"], cfg["nfeats"], cfg["num_actions"], True, "rot6d", True, True,
                     num_frames=cfg["num_frames"], latent_dim=cfg["latent_dim"], ff_size=cfg["ff_size"],
                     num_layers=cfg["layers"], num_heads=cfg["num_heads"], dropout=0.1, activation="gelu",
                     data_rep="rot6d", dataset=cfg["dataset"], arch="gru", cm_mode=cfg["cm_mode"],
                     body_model="smplx", cond_mode=cfg["cond_mode"], cond_mask_prob=cfg["cond_mask_prob"],
                     action_emb="tensor", emb_trans_dec=False, wo_pos_emb=False)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    assert not unexpected, unexpected
    assert all(k.startswith("clip_model.") for k in missing), missing
    model.eval()
    if scan == "frames":
        model.gru = _OverFrames(model.gru)
    else:
        assert scan == "batch"
    if "text" in cfg["cond_mode"]:   # CLIP is out of scope: the text encoder output is an INPUT
        holder = {}
        model.encode_text = lambda raw_text: holder["feat"]
        model._feat_holder = holder
    diffusion = SpacedDiffusion(use_timesteps=space_timesteps(1000, resp or [1000]),
                                betas=gd.get_named_beta_schedule("cosine", 1000, 1.0),
                                model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                                loss_type=gd.LossType.MSE, rescale_timesteps=False, data_rep="rot6d", num_person=1,
                                body_model="smplx")
    return model, diffusion


def in_range(name, a):
    m = float(np.abs(a).max())
    assert 1.0 <= m <= 4.0, f"{name}: max-abs {m:.3f} outside [1, 4] - rescale the synthetic weights (synth.GRU_GAIN / GRU_OUT_GAIN)"
    return m


def gen_keys():
    out = {}
    for name in ("tiny_gru", "tiny_add_gru", "tiny_text_gru", "ntu_gru"):
        cfg = synth.get_config(name)
        model, _ = build_gru(cfg, synth.make_state_dict(cfg, seed=0))
        out[name] = {k: list(v.shape) for k, v in model.state_dict().items() if not k.startswith("clip_model.")}
    path = os.path.join(HERE, "gru_arch_keys.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote", path)


def gen_forward(name):
    cfg_name, B, ts, guided, uncond_ts, mixed, scan = FORWARD[name]
    cfg = synth.get_config(cfg_name)
    sd = synth.make_state_dict(cfg, seed=0)
    model, _ = build_gru(cfg, sd, scan=scan)
    y = make_y(cfg, B, guided)
    if "text" in cfg["cond_mode"]:
        model._feat_holder["feat"] = y["text_features"]
    x = torch.from_numpy(synth.make_noise_tape(cfg, B, 0, seed=11)[0])
    if guided:
        from model.cfg_sampler import ClassifierFreeSampleModel
        fmodel = ClassifierFreeSampleModel(model)
    else:
        fmodel = model
    with torch.no_grad():
        outs = [fmodel(x, torch.tensor([t] * B), y=y).numpy() for t in ts]
        outs_u = [model(x, torch.tensor([t] * B), y=dict(y, uncond=True)).numpy() for t in uncond_ts]
    kw = dict(cfg_name=cfg_name, over=repr({}), scan=scan, B=B, ts=np.array(ts), guided=guided, out=np.stack(outs),
              sd_digest=sd_digest(sd), in_digest=digest(x.numpy(), y["cmotion"].numpy()))
    if mixed:                                                        # a different timestep per sample
        tmix = torch.tensor([(0, 999, 37, 500)[i % 4] for i in range(B)])
        with torch.no_grad():
            kw.update(t_mixed=tmix.numpy(), out_mixed=fmodel(x, tmix, y=y).numpy())
    if uncond_ts:
        kw.update(uncond_ts=np.array(uncond_ts), out_uncond=np.stack(outs_u))
    print(f"{name}: max-abs {in_range(name, kw['out']):.3f}")
    save(name, **kw)


def gen_loop(name):
    cfg_name, B, resp, mode, guided, inpaint, scan = LOOPS[name]
    cfg = synth.get_config(cfg_name)
    sd = synth.make_state_dict(cfg, seed=0)
    model, diffusion = build_gru(cfg, sd, resp, scan)
    S = diffusion.num_timesteps
    y = make_y(cfg, B, guided)
    if "text" in cfg["cond_mode"]:
        model._feat_holder["feat"] = y["text_features"]
    extra = {}
    if inpaint:
        mask, target = inpaint_inputs(cfg, B)
        y["inpainting_mask"] = torch.from_numpy(mask)
        y["inpainted_motion"] = torch.from_numpy(target)
        extra["inpaint_digest"] = digest(mask, target)
    tape = synth.make_noise_tape(cfg, B, S, seed=10)
    if guided:
        from model.cfg_sampler import ClassifierFreeSampleModel
        fmodel = ClassifierFreeSampleModel(model)
    else:
        fmodel = model
    shape = (B, cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    fn = diffusion.p_sample_loop if mode == "ddpm" else diffusion.ddim_sample_loop
    t0 = time.time()
    with _ref_import.NoiseTape(tape) as nt, torch.no_grad():
        final = fn(fmodel, shape, clip_denoised=False, model_kwargs={"y": y})
        assert nt.pos == S + 1, (nt.pos, S)
    dt = time.time() - t0
    print(f"{name}: reference {mode} S={S} B={B} took {dt:.1f}s, max-abs {in_range(name, final.numpy()):.3f}")
    save(name, cfg_name=cfg_name, over=repr({}), opts=repr({}), scan=scan, B=B, resp=resp, mode=mode, guided=guided, S=S, final=final.numpy(), ref_seconds=dt,
         sd_digest=sd_digest(sd), in_digest=digest(tape[0], tape[-1], y["cmotion"].numpy()), **extra)


JOBS = {"keys": gen_keys}
JOBS.update({n: (lambda n=n: gen_forward(n)) for n in FORWARD})
JOBS.update({n: (lambda n=n: gen_loop(n)) for n in LOOPS})

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    torch.set_num_threads(8)
    for k, fn in JOBS.items():
        if a.only is None or a.only == k:
            fn()
