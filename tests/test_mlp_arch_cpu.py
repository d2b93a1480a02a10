"""CPU: arch='mlp' (the reference's DiffMLP time / feature mixer, model/cmdm.py:239-242) - the fp32 restatement tests/mlp_arch_ref.py against
every golden recorded from the reference (tests/golden/make_golden_mlp.py), the parameter containers of CMDM(arch='mlp') against the
reference's state dict, and what the model refuses."""
import json
import os

import numpy as np
import pytest
import torch

from regennet_amd import synth
from regennet_amd.model.cmdm import CMDM
from tests import mlp_arch_ref
from tests.helpers import fixture_inputs
from tests.mlp_arch_cases import FORWARD, LOOPS, inpaint_inputs

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _model(cfg, **kw):
    return CMDM("", cfg["njoints"], cfg["nfeats"], cfg["num_actions"], True, "rot6d", True, True, num_frames=cfg["num_frames"],
                latent_dim=cfg["latent_dim"], ff_size=cfg["ff_size"], num_layers=cfg["layers"], num_heads=cfg["num_heads"],
                arch=kw.pop("arch", cfg.get("arch", "online")), cm_mode=cfg["cm_mode"], body_model="smplx", cond_mode=cfg["cond_mode"],
                cond_mask_prob=cfg["cond_mask_prob"], dataset=cfg["dataset"], **kw)


@pytest.mark.parametrize("name", sorted(FORWARD))
def test_restatement_matches_the_reference_forward(name):
    g = _golden(name)
    cfg, sd, y, x = fixture_inputs(g, loop=False)
    yt = {k: torch.from_numpy(np.asarray(v)) for k, v in y.items()}
    fwd = mlp_arch_ref.cfg_forward if bool(g["guided"]) else mlp_arch_ref.cmdm_forward
    B = x.shape[0]
    xt = torch.from_numpy(x)
    for i, t in enumerate(g["ts"]):
        err = float(np.abs(fwd(sd, cfg, xt, torch.full((B,), int(t)), yt).numpy() - g["out"][i]).max())
        assert err <= 1e-5, (name, int(t), err)
    for i, t in enumerate(g.get("uncond_ts", [])):
        err = float(np.abs(mlp_arch_ref.cmdm_forward(sd, cfg, xt, torch.full((B,), int(t)), dict(yt, uncond=True)).numpy() - g["out_uncond"][i]).max())
        assert err <= 1e-5, (name, "uncond", int(t), err)
    if "t_mixed" in g:
        err = float(np.abs(fwd(sd, cfg, xt, torch.from_numpy(g["t_mixed"]), yt).numpy() - g["out_mixed"]).max())
        assert err <= 1e-5, (name, "mixed", err)


def test_goldens_are_order_one():
    """The synthetic weights are scaled so that every recorded output has max-abs in [1, 4]: the absolute bounds of the GPU tests mean something."""
    for name in FORWARD:
        assert 1.0 <= float(np.abs(_golden(name)["out"]).max()) <= 4.0, name
    for name in LOOPS:
        assert 1.0 <= float(np.abs(_golden(name)["final"]).max()) <= 4.0, name


def test_inpaint_golden_inputs_rebuild():
    from tests.helpers import digest
    g = _golden("mlp_tiny_inpaint_ddpm10")
    mask, target = inpaint_inputs(synth.get_config(str(g["cfg_name"])), int(g["B"]))
    assert digest(mask, target) == str(g["inpaint_digest"])


@pytest.mark.parametrize("name", ["tiny_mlp", "tiny_add_mlp", "ntu_mlp"])
def test_state_dict_keys_and_shapes_equal_the_reference(name):
    with open(os.path.join(GOLDEN, "mlp_keys.json")) as f:
        want = json.load(f)[name]
    cfg = synth.get_config(name)
    got = {k: list(v.shape) for k, v in _model(cfg).state_dict().items()}
    assert got == want
    sd = synth.make_state_dict(cfg, seed=0)
    assert {k: list(v.shape) for k, v in sd.items()} == want                       # ... and the synthetic checkpoint draws exactly these
    assert list(sd["mlp.motion_mlp.mlps.0.fc0.weight"].shape) == [cfg["num_frames"], cfg["num_frames"], 1]


def test_concat_checkpoint_with_unused_fuse_process_loads():
    cfg = synth.get_config("tiny_mlp")
    assert cfg["cm_mode"] == "concat"
    sd = synth.make_state_dict(cfg, seed=0)
    assert "fuse_process.weight" in sd
    missing, unexpected = _model(cfg).load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not missing and not unexpected


def test_engine_config_carries_the_arch():
    from regennet_amd import _lib
    cfg = synth.get_config("tiny_mlp")
    assert _model(cfg).engine_config()["arch"] == "mlp" and _lib.ARCH["mlp"] == 3


def test_gru_still_refuses():
    with pytest.raises(NotImplementedError, match="gru"):
        _model(synth.get_config("tiny"), arch="gru")


def test_other_frame_count_raises_value_error_naming_fc0():
    cfg = synth.get_config("tiny_mlp")
    model = _model(cfg)
    with pytest.raises(ValueError, match="fc0"):
        model._get_engine(1, cfg["num_frames"] + 1)
    x = torch.zeros(1, cfg["njoints"], cfg["nfeats"], cfg["num_frames"] + 1)
    with pytest.raises(ValueError, match="fc0"):
        mlp_arch_ref.cmdm_forward(synth.make_state_dict(cfg), cfg, x, torch.zeros(1, dtype=torch.long), {"cmotion": x})


@pytest.mark.parametrize("tool", ["cgenerate", "edit", "score", "score_bpd"])
def test_command_line_tools_parse_arch_mlp_and_build_the_model(tool):
    """--arch mlp on every command line that parses --arch, through the factory call the tools make (allow_mlp=True); the factory's
    two-argument form keeps refusing the architecture."""
    import inspect
    import types
    from regennet_amd.eval import score
    from regennet_amd.sample import cgenerate, edit
    from regennet_amd.utils import parser_util
    from regennet_amd.utils.model_util import create_model_and_diffusion
    argv = ["--arch", "mlp", "--dataset", "ntu", "--unconstrained"]
    args = {"cgenerate": parser_util.cgenerate_args, "edit": parser_util.edit_args, "score": parser_util.score_args,
            "score_bpd": lambda a: parser_util.score_args(a + ["--bpd"])}[tool](argv)
    assert args.arch == "mlp"
    data = types.SimpleNamespace(dataset=types.SimpleNamespace(num_actions=26, num_person=2))
    model, diffusion = create_model_and_diffusion(args, data, allow_mlp=True)
    assert model.arch == "mlp" and model.engine_config()["arch"] == "mlp"
    assert any(k.startswith("mlp.motion_mlp.mlps.0.conct") for k in model.state_dict())
    with pytest.raises(NotImplementedError, match="allow_mlp"):
        create_model_and_diffusion(args, data)
    module = {"cgenerate": cgenerate, "edit": edit}.get(tool, score)
    assert "create_model_and_diffusion(args, data, allow_mlp=True)" in inspect.getsource(module)
