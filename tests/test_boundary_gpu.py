"""GPU: the sampler step has ONE definition (regennet_amd/csrc/rgn_sampler.h) behind the three kernels that run it - k_update, k_step and
the step boundary of k_layers<true>.

With an all-True in-painting mask pred_xstart is the bound target whatever the network computed, so the state after a step depends only on
the boundary arithmetic (select, clamp, DDPM / DDIM lines), the noise stream and the coefficient table: every form of the boundary must then
give the same bits. Each case runs the first S - 1 of S = 8 steps (the last step returns x0 alone and would hide the update) through
rgn_sample_range in the plain phase (no split-bf16 tail), on the four forms below, and compares x and x0_out with torch.equal. The planned
kernel names are asserted first, so the comparison cannot pass by running one kernel four times."""
import functools

import numpy as np
import pytest
import torch

from regennet_amd import synth
from tests.helpers import build_hip, y_to_device

pytestmark = pytest.mark.gpu

B, S = 3, 8
FORMS = {                                   # engine options -> the kernel that runs the step boundary
    "k_update": {"NO_STEP_FUSION": 1},
    "k_step": {"LAYERS": 0},
    "k_layers<false> + k_step": {"LAYERS_MIN_B": 1, "LAYERS_STEPS": 0},
    "k_layers<true>": {"LAYERS_MIN_B": 1, "LAYERS_GUIDED": 2},
}


def _planned(form, guided, f16):
    """(names that must be planned, names that must not) for the plain phase of a form."""
    step = "k_step<guided>" if guided else "k_step"
    steps = ("k_layers<true, true, f16>" if guided else "k_layers<true, false, f16>") if f16 else ("k_layers<true, true>" if guided else "k_layers<true>")
    every = {"k_update", "k_step", "k_step<guided>", "k_layers<false>", "k_layers<true>", "k_layers<true, true>", "k_layers<true, false, f16>",
             "k_layers<true, true, f16>"}
    want = {"k_update": {"k_update"}, "k_step": {step}, "k_layers<false> + k_step": {"k_layers<false>", step}, "k_layers<true>": {steps}}[form]
    return want, every - want


@functools.lru_cache(maxsize=None)
def _inputs(cfg_name, T):
    cfg = synth.get_config(cfg_name, num_frames=T)
    sd = synth.make_state_dict(cfg, seed=0)
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=7)}
    guided = "action" in cfg["cond_mode"]
    if guided:
        y["action"] = synth.make_actions(cfg, B, seed=2)
        y["scale"] = np.linspace(1.5, 3.5, B).astype(np.float32)
    tape = torch.from_numpy(synth.make_noise_tape(cfg, B, S, seed=8)).cuda()
    target = synth.make_noise_tape(cfg, B, 0, seed=12)[0]                    # (tests/inpaint_cases.py: x target_scale)
    targets = [torch.from_numpy((target * np.float32(s)).astype(np.float32)).cuda().contiguous() for s in (0.5, 1.5)]
    return cfg, sd, y, guided, tape, targets


_ENGINES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for model, _, _ in _ENGINES.values():
        model._engine.close()
    _ENGINES.clear()


def _engine(cfg_name, T, form, f16_steps):
    """One engine per (model, form), kept for the module: bound to its condition and schedule, its planned kernels checked."""
    key = (cfg_name, T, form, f16_steps)
    if key not in _ENGINES:
        _ENGINES[key] = _build_engine(*key)
    return _ENGINES[key]


def _build_engine(cfg_name, T, form, f16_steps):
    cfg, sd, y, guided, _, _ = _inputs(cfg_name, T)
    model, diffusion = build_hip(cfg, sd, resp=str(S), precision="bf16_x3tail/throughput", x3_tail=0, engine_options=FORMS[form], f16_steps=f16_steps)
    fm = model
    if guided:
        from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
        fm = ClassifierFreeSampleModel(model)
    eng, g, _ = fm._rgn_bind(B, y_to_device(y), None, T=T)
    assert bool(g) == guided
    eng.set_schedule(diffusion.timestep_map, diffusion._engine_tables(), diffusion._sched_token)
    n16 = 0 if form == "k_update" else f16_steps          # (the fp16 sub-phase belongs to the fused boundary: rgn_plan.cpp prec_plan)
    assert eng.precision_plan(B, guided) == (n16, 0), "every step is a plain-phase step"
    names = {rec["kernel"] for cls, rec in eng.plan_query(B, guided, split_phase=False).items() if rec["launches_per_eval"] > 0 or cls == "steps_fused"}
    want, never = _planned(form, guided, f16_steps > 0)
    assert want <= names and not (never & names), (form, sorted(names))
    return model, eng, guided


def _run(cfg_name, T, form, f16_steps, sampler, eta, clip, noise, const_noise, target):
    """(x, x0_out) after the first S - 1 steps with an all-True mask over `target`."""
    _, _, _, _, tape, _ = _inputs(cfg_name, T)
    _, eng, guided = _engine(cfg_name, T, form, f16_steps)
    st = torch.cuda.current_stream().cuda_stream
    x, x0 = tape[0].clone(), torch.zeros_like(tape[0])
    mask = torch.ones(tuple(x.shape), dtype=torch.bool, device="cuda")
    eng.set_const_noise(const_noise)
    eng.set_inpainting(mask, target, st)
    try:
        eng.sample_range(sampler, guided, eta, x, tape[1:] if noise == "tape" else None, 21, 100, S - 1, S - 1, x0, False, clip, st)
        torch.cuda.synchronize()
    finally:
        eng.set_const_noise(False)
        eng.clear_inpainting()
    return x, x0


SAMPLERS = {"ddpm": ("ddpm", 0.0), "ddim_eta1": ("ddim", 1.0), "ddim_eta0": ("ddim", 0.0)}
CASES = [(c, T, s, clip, "philox", False, 0) for c in ("ntu", "ntu_action") for T in (60, 57) for s in SAMPLERS for clip in (True, False)]
CASES += [("ntu_action", 57, "ddpm", True, "tape", False, 0),          # a noise tape instead of the Philox draw
          ("ntu", 60, "ddpm", False, "philox", True, 0),               # const_noise: motion 0's draw for every motion
          ("ntu_action", 60, "ddim_eta1", True, "philox", False, 8)]   # f16_steps = 8: the fp16-operand forms on every step


@pytest.mark.parametrize("cfg_name,T,sampler,clip,noise,const_noise,f16_steps", CASES)
def test_step_boundary_forms_agree_bit_for_bit(cfg_name, T, sampler, clip, noise, const_noise, f16_steps):
    """T = 60: every quad of lanes is a run of four frames, so k_step and k_layers<true> draw per quad; T = 57: they draw per element and
    k_step's 64-row tiles straddle samples. Target 0.5 x stays inside [-1, 1]; 1.5 x is clamped when clip is on."""
    name, eta = SAMPLERS[sampler]
    for target in _inputs(cfg_name, T)[5]:
        got = {form: _run(cfg_name, T, form, f16_steps, name, eta, clip, noise, const_noise, target) for form in FORMS}
        want0 = target.clamp(-1, 1) if clip else target
        x_ref, x0_ref = got["k_update"]
        assert torch.isfinite(x_ref).all() and not torch.equal(x_ref, x0_ref), "the state after a step is not x0: the update ran"
        for form, (x, x0) in got.items():
            assert torch.equal(x0, want0), (form, "pred_xstart is the (clamped) target")
            assert torch.equal(x, x_ref), (form, float((x - x_ref).abs().max()))
