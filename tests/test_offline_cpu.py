"""CPU: the arch='offline' surface - model construction with the reference's encoder keys, the C-ABI config field and its
argument check, and the fp32 CPU restatement (tests/offline_ref.py) against goldens recorded from the reference."""
import ctypes
import json
import os
import types
from unittest import mock

import numpy as np
import pytest
import torch

from oracle import regennet_oracle as orc
from regennet_amd import synth
from tests import offline_ref
from tests.helpers import autoreg_inputs, fixture_inputs

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _args(**over):
    from regennet_amd.utils.parser_util import cgenerate_args
    a = cgenerate_args(["--unconstrained", "--arch", "offline"])
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_offline_model_has_the_reference_encoder_keys():
    from regennet_amd.utils import model_util
    ref = json.load(open(os.path.join(GOLDEN, "offline_keys.json")))["ntu_offline"]
    data = types.SimpleNamespace(dataset=types.SimpleNamespace(num_actions=26, num_person=2))
    model, _ = model_util.create_model_and_diffusion(_args(), data)
    assert model.arch == "offline" and model.engine_config()["arch"] == "offline"
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert got == ref
    assert not any(k.startswith("seqTransDecoder.") or ".multihead_attn." in k or ".norm3." in k for k in got)


def test_synth_offline_checkpoints_use_the_reference_key_set():
    ref = json.load(open(os.path.join(GOLDEN, "offline_keys.json")))
    for name in ("tiny_offline", "ntu_offline"):
        sd = synth.make_state_dict(synth.get_config(name), seed=0)
        assert {k: list(v.shape) for k, v in sd.items()} == ref[name]


@pytest.mark.parametrize("arch", ["trans_enc", "gru", "mlp"])
def test_other_architectures_still_refused(arch):
    from regennet_amd.utils import model_util
    data = types.SimpleNamespace(dataset=types.SimpleNamespace(num_actions=26, num_person=2))
    with pytest.raises(NotImplementedError):
        model_util.create_model_and_diffusion(_args(arch=arch), data)


@pytest.mark.parametrize("model_arch,ckpt", [("offline", "tiny"), ("online", "tiny_offline")])
def test_online_and_offline_checkpoints_do_not_cross_load(model_arch, ckpt):
    from regennet_amd.model.cmdm import CMDM
    from regennet_amd.utils.model_util import load_model_wo_clip
    cfg = synth.get_config("tiny")
    model = CMDM("", cfg["njoints"], cfg["nfeats"], cfg["num_actions"], True, "rot6d", True, True, num_frames=cfg["num_frames"],
                 latent_dim=cfg["latent_dim"], ff_size=cfg["ff_size"], num_layers=cfg["layers"], num_heads=cfg["num_heads"],
                 arch=model_arch, cm_mode=cfg["cm_mode"], cond_mode=cfg["cond_mode"], cond_mask_prob=0.1, action_emb="tensor")
    sd = synth.make_state_dict(synth.get_config(ckpt), seed=0)
    with pytest.raises(Exception):
        load_model_wo_clip(model, {k: torch.from_numpy(v) for k, v in sd.items()})


def test_rgn_config_ends_in_arch_and_bad_arch_is_refused_before_the_device_check():
    from regennet_amd import _lib
    assert _lib.RgnConfig._fields_[-1][0] == "arch"
    assert ctypes.sizeof(_lib.RgnConfig) == 17 * 4
    lib = _lib.load()
    cfg = _lib.RgnConfig(njoints=56, nfeats=6, num_frames=60, latent_dim=512, ff_size=1024, num_heads=4, num_layers=8, cm_mode=1,
                         cond_mode=0, num_actions=1, clip_dim=512, emb_trans_dec=0, wo_pos_emb=0, max_batch=1, precision=0, device=0,
                         arch=2)
    h = ctypes.c_void_p()
    assert lib.rgn_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    assert b"arch" in lib.rgn_last_error(None)


@pytest.mark.parametrize("name", ["offline_tiny_fwd", "offline_tiny_fwd_cfg", "offline_ntu_fwd", "offline_chi3d_fwd"])
def test_offline_ref_matches_the_forward_goldens(name):
    g = _golden(name)
    cfg, sd, y, x = fixture_inputs(g, loop=False)
    yt = {k: torch.from_numpy(np.asarray(v)) for k, v in y.items()}
    fwd = offline_ref.cfg_forward if bool(g["guided"]) else offline_ref.cmdm_forward
    xt = torch.from_numpy(x)
    B = x.shape[0]
    # fp32 on both sides; at d = 512 / 8 layers the CPU GEMMs' summation order differs from the reference's batched call (measured
    # 3.5e-6 at 61 and 1.0e-5 at 151 tokens), the bound the online oracle test applies to its forward goldens
    tol = 1e-5 if cfg["latent_dim"] <= 64 else 2e-5
    for i, t in enumerate(g["ts"]):
        out = fwd(sd, cfg, xt, torch.full((B,), int(t), dtype=torch.long), yt).numpy()
        assert np.abs(out - g["out"][i]).max() <= tol, (name, int(t))
    for i, t in enumerate(g.get("uncond_ts", [])):
        out = offline_ref.cmdm_forward(sd, cfg, xt, torch.full((B,), int(t), dtype=torch.long), dict(yt, uncond=True)).numpy()
        assert np.abs(out - g["out_uncond"][i]).max() <= tol, (name, "uncond", int(t))


@pytest.mark.parametrize("name", ["offline_tiny_add_ddpm10", "offline_tiny_ddim10_cfg"])
def test_offline_ref_through_the_oracle_sampling_loop(name):
    g = _golden(name)
    cfg, sd, y, tape = fixture_inputs(g, loop=True)
    sched = orc.make_schedule("cosine", str(g["resp"]))
    yt = {k: torch.from_numpy(np.asarray(v)) for k, v in y.items()}
    with mock.patch.object(orc, "cmdm_forward", offline_ref.cmdm_forward):
        out = orc.sample_loop(sd, cfg, sched, tape, yt, mode=str(g["mode"]), guided=bool(g["guided"])).numpy()
    assert np.abs(out - g["final"]).max() <= 1e-4, name
