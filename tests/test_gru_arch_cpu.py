"""CPU: arch='gru' (the reference's nn.GRU denoiser, model/cmdm.py:191-199, 243-249) - the restatement tests/gru_arch_ref.py against every golden
recorded from the reference (tests/golden/make_golden_gru_arch.py) in both scans, the parameter containers of CMDM(arch='gru') against the
reference's state dict, the command lines, what the model and the library refuse without a device, and the mutants that the GPU bounds must catch."""
import ctypes
import functools
import json
import os
import types
from unittest import mock

import numpy as np
import pytest
import torch

from oracle import regennet_oracle as orc
from regennet_amd import _lib, synth
from regennet_amd.model.cmdm import CMDM
from tests import gru_arch_ref
from tests.gru_arch_cases import FORWARD, LOOPS, inpaint_inputs
from tests.helpers import digest, fixture_inputs

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
GPU_BOUND = 1e-3                                   # the widest bound tests/test_gru_arch_gpu.py applies (split-bf16 modes; f32: 2e-4)


def _golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _model(cfg, **kw):
    return CMDM("", cfg["njoints"], cfg["nfeats"], cfg["num_actions"], True, "rot6d", True, True, num_frames=cfg["num_frames"],
                latent_dim=cfg["latent_dim"], ff_size=cfg["ff_size"], num_layers=cfg["layers"], num_heads=cfg["num_heads"],
                arch=kw.pop("arch", cfg.get("arch", "online")), cm_mode=kw.pop("cm_mode", cfg["cm_mode"]), body_model="smplx", cond_mode=cfg["cond_mode"],
                cond_mask_prob=cfg["cond_mask_prob"], dataset=cfg["dataset"], **kw)


def _forward_errors(name, mutant=None):
    """max |restatement - golden| over every recorded call of a forward fixture."""
    g = _golden(name)
    cfg, sd, y, x = fixture_inputs(g, loop=False)
    scan = str(g["scan"])
    assert scan == FORWARD[name][6]
    yt = {k: torch.from_numpy(np.asarray(v)) for k, v in y.items()}
    fwd = functools.partial(gru_arch_ref.cfg_forward if bool(g["guided"]) else gru_arch_ref.cmdm_forward, scan=scan, mutant=mutant)
    B = x.shape[0]
    xt = torch.from_numpy(x)
    errs = [float(np.abs(fwd(sd, cfg, xt, torch.full((B,), int(t)), yt).numpy() - g["out"][i]).max()) for i, t in enumerate(g["ts"])]
    for i, t in enumerate(g.get("uncond_ts", [])):
        out = gru_arch_ref.cmdm_forward(sd, cfg, xt, torch.full((B,), int(t)), dict(yt, uncond=True), scan=scan, mutant=mutant)
        errs.append(float(np.abs(out.numpy() - g["out_uncond"][i]).max()))
    if "t_mixed" in g:
        errs.append(float(np.abs(fwd(sd, cfg, xt, torch.from_numpy(g["t_mixed"]), yt).numpy() - g["out_mixed"]).max()))
    return cfg, max(errs)


@pytest.mark.parametrize("name", sorted(FORWARD))
def test_restatement_matches_the_reference_forward(name):
    cfg, err = _forward_errors(name)
    assert err <= (1e-5 if cfg["latent_dim"] <= 64 else 2e-5), (name, err)         # the bound tests/test_offline_cpu.py uses


@pytest.mark.parametrize("name", sorted(n for n in LOOPS if not LOOPS[n][5]))
def test_restatement_through_the_oracle_sampling_loop(name):
    g = _golden(name)
    cfg, sd, y, tape = fixture_inputs(g, loop=True)
    yt = {k: torch.from_numpy(np.asarray(v)) for k, v in y.items()}
    with mock.patch.object(orc, "cmdm_forward", functools.partial(gru_arch_ref.cmdm_forward, scan=str(g["scan"]))):
        out = orc.sample_loop(sd, cfg, orc.make_schedule("cosine", str(g["resp"])), tape, yt, mode=str(g["mode"]), guided=bool(g["guided"])).numpy()
    assert np.abs(out - g["final"]).max() <= 1e-4, name


def test_goldens_are_order_one():
    """The synthetic weights are scaled so that every recorded output has max-abs in [1, 4]: the absolute bounds of the GPU tests mean something."""
    for name in FORWARD:
        assert 1.0 <= float(np.abs(_golden(name)["out"]).max()) <= 4.0, name
    for name in LOOPS:
        assert 1.0 <= float(np.abs(_golden(name)["final"]).max()) <= 4.0, name


def test_inpaint_golden_inputs_rebuild():
    g = _golden("gru_arch_tiny_inpaint_ddpm10")
    mask, target = inpaint_inputs(synth.get_config(str(g["cfg_name"])), int(g["B"]))
    assert digest(mask, target) == str(g["inpaint_digest"])


# ---- mutants: each mistake must leave the GPU bound on at least one fixture, or the fixtures could not catch it
@pytest.mark.parametrize("mutant", gru_arch_ref.MUTANTS)
def test_every_mutant_violates_the_gpu_bound_on_some_fixture(mutant):
    worst = {name: _forward_errors(name, mutant)[1] for name in sorted(FORWARD) if name != "gru_arch_ntu_fwd"}
    print(f"\n[gru mutant] {mutant}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) > GPU_BOUND, (mutant, worst)
    if mutant == "other_axis":                       # the recurrence matters in BOTH scans: the synthetic gains do not let the state die out
        assert worst["gru_arch_tiny_fwd"] > GPU_BOUND and worst["gru_arch_tiny_fwd_frames"] > GPU_BOUND, worst
    if mutant == "no_restart":                       # only a guided batch scan has a boundary to restart at
        assert worst["gru_arch_tiny_fwd_cfg"] > GPU_BOUND and worst["gru_arch_tiny_fwd"] == _forward_errors("gru_arch_tiny_fwd")[1]


def test_batch_scan_couples_later_samples_and_no_other_frame():
    """The reference's recurrence: changing sample 1 at frame 3 changes samples 1, 2, 3 at frame 3 and nothing else."""
    cfg = synth.get_config("tiny_add_gru")
    sd = synth.make_state_dict(cfg, seed=0)
    B = 4
    x = torch.from_numpy(synth.make_noise_tape(cfg, B, 0, seed=11)[0])
    y = {"cmotion": torch.from_numpy(synth.make_cmotion(cfg, B, seed=1))}
    t = torch.full((B,), 300)
    a = gru_arch_ref.cmdm_forward(sd, cfg, x, t, y)
    x2 = x.clone()
    x2[1, :, :, 3] += 1.0
    b = gru_arch_ref.cmdm_forward(sd, cfg, x2, t, y)
    changed = (a != b).any(dim=1).any(dim=1)         # [B, T]
    want = torch.zeros_like(changed)
    want[1:, 3] = True
    assert torch.equal(changed, want)


# ---- the model
@pytest.mark.parametrize("name", ["tiny_gru", "tiny_add_gru", "tiny_text_gru", "ntu_gru"])
def test_state_dict_keys_and_shapes_equal_the_reference(name):
    with open(os.path.join(GOLDEN, "gru_arch_keys.json")) as f:
        want = json.load(f)[name]
    cfg = synth.get_config(name)
    assert cfg["arch"] == "gru" and cfg["cm_mode"] == "add"
    got = {k: list(v.shape) for k, v in _model(cfg).state_dict().items()}
    assert got == want
    assert list(got) == list(_model(cfg).state_dict())                            # (and nn.GRU's own key order)
    sd = synth.make_state_dict(cfg, seed=0)
    assert {k: list(v.shape) for k, v in sd.items()} == want                       # ... and the synthetic checkpoint draws exactly these
    d, F = cfg["latent_dim"], cfg["njoints"] * cfg["nfeats"]
    assert want["input_process.poseEmbedding.weight"] == [d, F + d] and want["gru.weight_hh_l1"] == [3 * d, d]
    assert not any(k.startswith("fuse_process.") for k in want)


def test_every_gru_config_is_the_base_config_with_arch_and_add():
    for base in ("tiny", "tiny_add", "tiny_text", "ntu", "ntu_action", "chi3d"):
        assert synth.get_config(base + "_gru") == dict(synth.get_config(base), arch="gru", cm_mode="add")


def test_model_builds_loads_and_carries_arch_and_scan():
    cfg = synth.get_config("tiny_gru")
    model = _model(cfg)
    assert model.arch == "gru" and model.engine_config()["arch"] == "gru" and _lib.ARCH["gru"] == 4 and model.gru_scan == "batch"
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=0).items()}, strict=False)
    assert not missing and not unexpected
    assert _model(cfg, gru_scan="frames").gru_scan == "frames"
    with pytest.raises(ValueError, match="gru_scan"):
        _model(cfg, gru_scan="diagonal")


@pytest.mark.parametrize("model_cfg,ckpt", [("tiny_gru", "tiny_add"), ("tiny_gru", "tiny_mlp"), ("tiny_add", "tiny_add_gru"), ("tiny_add_mlp", "tiny_add_gru")])
def test_checkpoints_of_other_architectures_do_not_cross_load(model_cfg, ckpt):
    from regennet_amd.utils.model_util import load_model_wo_clip
    model = _model(synth.get_config(model_cfg))
    sd = synth.make_state_dict(synth.get_config(ckpt), seed=0)
    with pytest.raises(Exception):
        load_model_wo_clip(model, {k: torch.from_numpy(v) for k, v in sd.items()})


def test_gru_with_another_cm_mode_still_raises_naming_gru():
    with pytest.raises(NotImplementedError, match="gru"):
        _model(synth.get_config("tiny_gru"), cm_mode="concat")
    with pytest.raises(NotImplementedError, match="add"):
        gru_arch_ref.cmdm_forward({}, dict(synth.get_config("tiny_gru"), cm_mode="concat"), torch.zeros(1, 5, 6, 8), torch.zeros(1, dtype=torch.long), {})


# ---- the command lines
@pytest.mark.parametrize("tool", ["cgenerate", "edit"])
@pytest.mark.parametrize("scan", ["batch", "frames"])
def test_command_line_tools_parse_arch_gru_and_build_the_model(tool, scan):
    import inspect
    from regennet_amd.sample import cgenerate, edit
    from regennet_amd.utils import parser_util
    from regennet_amd.utils.model_util import create_model_and_diffusion
    argv = ["--arch", "gru", "--cm_mode", "add", "--gru_scan", scan, "--dataset", "ntu", "--unconstrained"]
    args = {"cgenerate": parser_util.cgenerate_args, "edit": parser_util.edit_args}[tool](argv)
    assert args.arch == "gru" and args.gru_scan == scan
    data = types.SimpleNamespace(dataset=types.SimpleNamespace(num_actions=26, num_person=2))
    model, diffusion = create_model_and_diffusion(args, data, allow_gru=True)
    assert model.arch == "gru" and model.gru_scan == scan and model.engine_config()["arch"] == "gru"
    assert "gru.weight_hh_l7" in model.state_dict()
    with pytest.raises(NotImplementedError, match="allow_gru"):
        create_model_and_diffusion(args, data)
    with pytest.raises(NotImplementedError, match="allow_gru"):
        create_model_and_diffusion(args, data, allow_mlp=True)
    assert "allow_gru=True" in inspect.getsource({"cgenerate": cgenerate, "edit": edit}[tool])


def test_gru_scan_defaults_to_the_reference_recurrence():
    from regennet_amd.utils import parser_util
    assert parser_util.cgenerate_args(["--arch", "gru", "--cm_mode", "add"]).gru_scan == "batch"


def test_score_refuses_arch_gru_and_says_why():
    from regennet_amd.eval import score
    with pytest.raises(NotImplementedError, match="batch scan"):
        score.main(["--arch", "gru", "--cm_mode", "add", "--dataset", "ntu", "--unconstrained", "--synthetic"])


# ---- the library, without a device
def _config(**over):
    kw = dict(njoints=5, nfeats=6, num_frames=8, latent_dim=64, ff_size=128, num_heads=4, num_layers=2, cm_mode=0, cond_mode=0, num_actions=1,
              clip_dim=512, emb_trans_dec=0, wo_pos_emb=0, max_batch=1, precision=0, device=0, arch=4)
    kw.update(over)
    return _lib.RgnConfig(**kw)


def test_abi_symbols_and_constants():
    lib = _lib.load()
    for name in ("rgn_set_gru_scan", "rgn_gru_stack_info"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert _lib.ARCH == {"online": 0, "offline": 1, "mlp": 3, "gru": 4} and _lib.GRU_SCAN == {"batch": 0, "frames": 1}
    assert _lib.RgnConfig._fields_[-1][0] == "arch" and ctypes.sizeof(_lib.RgnConfig) == 17 * 4
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "regennet_hip.h")).read()
    assert "RGN_ARCH_GRU = 4" in header and "rgn_set_gru_scan" in header and "RGN_GRU_SCAN_FRAMES = 1" in header


@pytest.mark.parametrize("over,code,word", [
    (dict(cm_mode=1), -7, b"cm_mode add"),                      # the reference's own refusal
    (dict(emb_trans_dec=1), -7, b"emb_trans_dec"),
    (dict(latent_dim=2048), -7, b"latent_dim"),
    (dict(num_layers=0), -1, b"non-positive"),
    (dict(arch=2), -1, b"arch"),                                # 2 stays unassigned
    (dict(arch=5), -1, b"arch"),
])
def test_create_refuses_before_the_device_check(over, code, word):
    lib = _lib.load()
    h = ctypes.c_void_p()
    cfg = _config(**over)
    assert lib.rgn_create(ctypes.byref(cfg), ctypes.byref(h)) == code
    assert word in lib.rgn_last_error(None), lib.rgn_last_error(None)
    assert not h.value


def test_scan_setter_and_info_refuse_a_null_handle():
    lib = _lib.load()
    assert lib.rgn_set_gru_scan(None, 0) == -1
    out = [ctypes.c_int32() for _ in range(4)]
    ws = ctypes.c_uint64()
    assert lib.rgn_gru_stack_info(None, 1, 0, *[ctypes.byref(o) for o in out], ctypes.byref(ws)) == -1
