"""GPU: ONE sampler step of every boundary form against the reference's own float32 arithmetic, element for element.

tests/test_boundary_gpu.py holds the four forms of the step boundary to each other; they share regennet_amd/csrc/rgn_sampler.h and the
coefficient table of rgn_plan.cpp, so a wrong line or an entry taken one index off leaves them equal, and the end-to-end bounds (1e-3 through a
network) are far too wide to notice. Here, with an all-True in-painting mask, pred_xstart is the bound target whatever the network computes: the
state after one rgn_sample_range step depends on the boundary arithmetic, the table and the noise alone, and is compared with
oracle.regennet_oracle.sampler_step (torch CPU float32 on orc.make_schedule's tables) under the bound of tests/sampler_step_ref.py:
|x' - ref| <= 2^-22 A. The planned kernel names are asserted, as in test_boundary_gpu.py.

Noise: a tape entry, or the engine's Philox draw - then the reference takes eps from rgn_randn_step of the same (seed, sample_offset, loop index),
which tests/test_noise_stream_gpu.py holds to the host statement of the stream.

Not covered here: guide(). The all-True mask overrides its result, so the guidance combination stays with the guided goldens."""
import functools

import numpy as np
import pytest
import torch

from regennet_amd import synth
from tests import sampler_step_ref as R
from tests.helpers import build_hip, y_to_device
from tests.test_boundary_gpu import FORMS, _planned

pytestmark = pytest.mark.gpu

B = 3
SEED, SAMPLE_OFFSET = 0x9E3779B97F4A7C15, 2 ** 32 - 2
MODELS = {"ntu60": ("ntu", 60), "ntu57": ("ntu", 57), "ntu_action60": ("ntu_action", 60)}
FULL_FORMS = ("k_update", "k_layers<true>")
CORE_FORMS = ("k_step", "k_layers<false> + k_step")


@functools.lru_cache(maxsize=None)
def _inputs(model):
    cfg_name, T = MODELS[model]
    cfg = synth.get_config(cfg_name, num_frames=T, layers=1)
    sd = synth.make_state_dict(cfg, seed=0)
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=7)}
    guided = "action" in cfg["cond_mode"]
    if guided:
        y["action"] = synth.make_actions(cfg, B, seed=2)
        y["scale"] = np.linspace(1.5, 3.5, B).astype(np.float32)
    tape = torch.from_numpy(synth.make_noise_tape(cfg, B, 8, seed=8))                  # [0]: the state x; [1 ..]: per-step tape entries
    target = torch.from_numpy(synth.make_noise_tape(cfg, B, 0, seed=12)[0])
    return cfg, sd, y, guided, tape, {s: (target * s).contiguous() for s in (0.5, 1.5)}


@functools.lru_cache(maxsize=None)
def _diffusion(schedule):
    """The project's own diffusion object of a schedule: what hands the engine its tables (the reference's come from orc.make_schedule)."""
    from regennet_amd.diffusion import gaussian_diffusion as gd
    from regennet_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    noise_schedule, resp, sigma_small = R.SCHEDULES[schedule]
    return SpacedDiffusion(use_timesteps=space_timesteps(1000, resp or [1000]), betas=gd.get_named_beta_schedule(noise_schedule, 1000, 1.0),
                           model_mean_type=gd.ModelMeanType.START_X,
                           model_var_type=gd.ModelVarType.FIXED_SMALL if sigma_small else gd.ModelVarType.FIXED_LARGE,
                           loss_type=gd.LossType.MSE, rescale_timesteps=False)


@functools.lru_cache(maxsize=None)
def _tables(schedule):
    tmap, tb = R.schedule(schedule)
    assert list(tmap) == list(_diffusion(schedule).timestep_map)
    return tb


_ENGINES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for model, _, _ in _ENGINES.values():
        model._engine.close()
    _ENGINES.clear()


def _engine(model, form, schedule):
    """The (model, form) engine bound to `schedule`: built once, its planned kernels checked, rebound with set_schedule per schedule."""
    key = (model, form)
    if key not in _ENGINES:
        cfg, sd, y, guided, _, _ = _inputs(model)
        m, _ = build_hip(cfg, sd, resp="8", precision="bf16_x3tail/throughput", x3_tail=0, engine_options=FORMS[form], f16_steps=0)
        fm = m
        if guided:
            from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
            fm = ClassifierFreeSampleModel(m)
        eng, g, _ = fm._rgn_bind(B, y_to_device(y), None, T=MODELS[model][1])
        assert bool(g) == guided
        _ENGINES[key] = (m, eng, guided)
    m, eng, guided = _ENGINES[key]
    d = _diffusion(schedule)
    if eng.schedule_id is not d._sched_token:
        eng.set_schedule(d.timestep_map, d._engine_tables(), d._sched_token)
        assert eng.precision_plan(B, guided) == (0, 0), "every step is a plain-phase step"
        names = {rec["kernel"] for cls, rec in eng.plan_query(B, guided, split_phase=False).items() if rec["launches_per_eval"] > 0 or cls == "steps_fused"}
        want, never = _planned(form, guided, False)
        assert want <= names and not (never & names), (form, sorted(names))
    return eng, guided


def _launch(eng, guided, sampler, eta, clip, x, target, first_index, count, tape=None, const_noise=False):
    """rgn_sample_range over `count` steps from loop index first_index with an all-True mask over `target`: (x', x0_out) on the host."""
    st = torch.cuda.current_stream().cuda_stream
    xd, x0d = x.cuda().contiguous(), torch.full(tuple(x.shape), float("nan"), device="cuda")
    mask = torch.ones(tuple(x.shape), dtype=torch.bool, device="cuda")
    eng.set_const_noise(const_noise)
    eng.set_inpainting(mask, target.cuda().contiguous(), st)
    try:
        eng.sample_range(sampler, guided, eta, xd, None if tape is None else tape.cuda().contiguous(), SEED, SAMPLE_OFFSET, first_index, count, x0d,
                         False, clip, st)
        torch.cuda.synchronize()
    finally:
        eng.set_const_noise(False)
        eng.clear_inpainting()
    return xd.cpu(), x0d.cpu()


def _philox_eps(eng, shape, loop_index, const_noise=False):
    """The draw rgn_sample_range adds at `loop_index` for (SEED, SAMPLE_OFFSET), re-drawn through rgn_randn_step."""
    buf = torch.empty(shape, device="cuda")
    eng.randn_step(buf, B, SEED, SAMPLE_OFFSET, loop_index, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    eps = buf.cpu()
    return eps[:1].expand(shape).contiguous() if const_noise else eps


def _check_steps(model, form, schedule, indices, samplers, const_noise_case=False):
    """Every (loop index, sampler, clip, target scale, noise source) of one (model, form, schedule): single-step launches from the same known x.
    Returns the largest |x' - ref| / A per sampler and the DDIM tape cases that were not bit-equal."""
    _, _, _, _, tape, targets = _inputs(model)
    tb = _tables(schedule)
    eng, guided = _engine(model, form, schedule)
    x = tape[0]
    worst, unequal, n = {}, [], 0
    for i in indices:
        eps_of = {"tape": tape[1 + i % 7], "philox": _philox_eps(eng, tuple(x.shape), i)}
        if const_noise_case:
            eps_of = {"philox_const": _philox_eps(eng, tuple(x.shape), i, const_noise=True)}
        for name in samplers:
            mode, eta = R.SAMPLERS[name]
            for clip in (True, False):
                for scale, target in targets.items():
                    for noise, eps in eps_of.items():
                        got, got0 = _launch(eng, guided, mode, eta, clip, x, target, i, 1, tape=eps[None] if noise == "tape" else None,
                                            const_noise=const_noise_case)
                        ref, ref0 = R.step_ref(tb, i, x, target, eps, mode, eta, clip)
                        case = (model, form, schedule, i, name, clip, scale, noise)
                        assert torch.equal(got0, ref0), (case, "x0_out is the (clamped) target")
                        assert torch.isfinite(got).all(), case
                        A = R.terms(tb, i, x, ref0, eps, mode, eta)
                        ratio = float(((got - ref).abs().double().numpy() / np.maximum(A, 1e-300)).max())
                        worst[mode] = max(worst.get(mode, 0.0), ratio)
                        if mode == "ddim" and noise == "tape" and not torch.equal(got, ref):
                            unequal.append(case)
                        assert ((got - ref).abs().double().numpy() <= R.BOUND * A).all(), (case, ratio / R.BOUND)
                        n += 1
    print(f"\n[sampler step] {model} {form} {schedule}: {n} single-step cases; max |x' - ref| / A: "
          + ", ".join(f"{m} {w:.3e} ({w / R.BOUND:.3f} of the bound)" for m, w in sorted(worst.items()))
          + f"; DDIM tape cases not bit-equal: {len(unequal)} {unequal[:4]}")
    return worst, unequal


@pytest.mark.parametrize("schedule", list(R.SCHEDULES))
@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("form", FULL_FORMS)
def test_one_step_against_the_reference_arithmetic(form, model, schedule):
    """The full grid on k_update and k_layers<true>: loop indices S - 1, S / 2, 2, 1, 0; ddpm and ddim at eta 0, 0.5, 1; clip on and off; target
    0.5 x (inside [-1, 1]) and 1.5 x (clamped when clip is on); a tape entry and the Philox draw; B = 3, sample_offset 2^32 - 2."""
    S = len(_tables(schedule)["betas"])
    _check_steps(model, form, schedule, R.loop_indices(S), list(R.SAMPLERS))


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("form", CORE_FORMS)
def test_one_step_core_on_the_other_forms(form, model):
    """k_step alone and behind k_layers<false>: cosine-1000, loop indices S - 1, 1, 0, both samplers (ddim at eta 0 and 1)."""
    _check_steps(model, form, "cosine1000", [999, 1, 0], ["ddpm", "ddim_eta0", "ddim_eta1"])


@pytest.mark.parametrize("form", list(FORMS))
def test_one_step_with_const_noise(form):
    """const_noise: every motion takes motion 0's draw (sample SAMPLE_OFFSET + 0)."""
    _check_steps("ntu57", form, "cosine_ddim5", [4, 1], ["ddpm", "ddim_eta1"], const_noise_case=True)


@pytest.mark.parametrize("noise", ("tape", "philox"))
@pytest.mark.parametrize("sampler", ("ddpm", "ddim_eta0.5"))
def test_seven_steps_in_one_launch(sampler, noise):
    """k_layers<true> carries a motion through runs of steps inside one launch: loop indices 7 .. 1 of cosine-8 (FIXED_LARGE) in a single
    rgn_sample_range call against the reference iterated 7 times. Bound: the sum of the per-step bounds - the x coefficient of either line is at
    most 1 in magnitude, so a step does not grow what earlier steps left."""
    model, form, schedule = "ntu57", "k_layers<true>", "cosine8_large"
    _, _, _, _, tape, targets = _inputs(model)
    tb = _tables(schedule)
    eng, guided = _engine(model, form, schedule)
    mode, eta = R.SAMPLERS[sampler]
    x, target = tape[0], targets[1.5]
    eps = tape[1:8] if noise == "tape" else torch.stack([_philox_eps(eng, tuple(x.shape), i) for i in range(7, 0, -1)])
    got, got0 = _launch(eng, guided, mode, eta, True, x, target, 7, 7, tape=eps if noise == "tape" else None)
    ref, bound = x, np.zeros(tuple(x.shape))
    for k, i in enumerate(range(7, 0, -1)):
        nxt, ref0 = R.step_ref(tb, i, ref, target, eps[k], mode, eta, True)
        bound += R.BOUND * R.terms(tb, i, ref, ref0, eps[k], mode, eta)
        ref = nxt
    err = (got - ref).abs().double().numpy()
    print(f"\n[sampler step] 7 steps in one launch, {sampler} {noise}: max |x' - ref| / bound = {float((err / bound).max()):.3f}, bit-equal: {torch.equal(got, ref)}")
    assert torch.equal(got0, target.clamp(-1, 1))
    assert torch.isfinite(got).all() and (err <= bound).all(), float((err / bound).max())
