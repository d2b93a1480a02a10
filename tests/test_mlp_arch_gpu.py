"""GPU: arch='mlp' (the reference's DiffMLP time / feature mixer, model/cmdm.py:239-242; rgn_mixer.hip) against goldens recorded from the
reference (tests/golden/make_golden_mlp.py) and against the fp32 CPU restatement tests/mlp_arch_ref.py, in every precision mode: forward and
sampling-loop parity, independence of the samples bit for bit, the plain phase, the refusals, and the scoring functions."""
import os

import numpy as np
import pytest
import torch

from regennet_amd import _lib, synth
from tests import mlp_arch_ref
from tests.helpers import build_hip, fixture_inputs, y_to_device
from tests.mlp_arch_cases import FORWARD, LOOPS, inpaint_inputs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PRECISIONS = ["f32", "bf16x3", "bf16_x3tail"]
TOL = {"f32": 2e-4, "bf16x3": 1e-3, "bf16_x3tail": 1e-3}     # the bounds tests/test_offline_gpu.py holds the other architectures to
TIME_KERNEL = {"f32": "k_mix_time<f32>", "bf16x3": "k_mix_time<bf16x3>", "bf16_x3tail": "k_mix_time<bf16x3>"}


def _golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _wrap(model, guided):
    if not guided:
        return model
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    return ClassifierFreeSampleModel(model)


def _close(model):
    for e in model._engines.values():
        e.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", sorted(FORWARD))
def test_mlp_forward_goldens(name, precision):
    """Every recorded timestep (0 and 999 among them), the y['uncond'] rows, and one rgn_denoise call with a different timestep per sample."""
    g = _golden(name)
    cfg, sd, y, x = fixture_inputs(g, loop=False)
    model, _ = build_hip(cfg, sd, precision=precision)
    fm = _wrap(model, bool(g["guided"]))
    yd, xd = y_to_device(y), torch.from_numpy(x).cuda()
    B = x.shape[0]
    errs = {}
    for i, t in enumerate(g["ts"]):
        out = fm(xd, torch.full((B,), int(t), dtype=torch.long, device="cuda"), y=yd)
        errs[int(t)] = float(np.abs(out.cpu().numpy() - g["out"][i]).max())
    for i, t in enumerate(g.get("uncond_ts", [])):
        out = model(xd, torch.full((B,), int(t), dtype=torch.long, device="cuda"), y=dict(yd, uncond=True))
        errs[f"uncond{int(t)}"] = float(np.abs(out.cpu().numpy() - g["out_uncond"][i]).max())
    if "t_mixed" in g:
        out = fm(xd, torch.from_numpy(g["t_mixed"]).cuda(), y=yd)
        errs["mixed"] = float(np.abs(out.cpu().numpy() - g["out_mixed"]).max())
    plan = model._engine.plan_query(B, guided=bool(g["guided"]), split_phase=True)
    _close(model)
    print(f"\n[mlp forward err] {name} {precision}: {errs}")
    assert plan["mixer"]["kernel"] == TIME_KERNEL[precision] and plan["mixer"]["launches_per_eval"] == cfg["layers"] + 2, plan
    assert max(errs.values()) < TOL[precision], (name, precision, errs)


def _loop(g, cfg, sd, y, tape, precision, **kw):
    model, diffusion = build_hip(cfg, sd, resp=str(g["resp"]), precision=precision, **kw)
    shape = (int(g["B"]), cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    fn = diffusion.p_sample_loop if str(g["mode"]) == "ddpm" else diffusion.ddim_sample_loop
    out = fn(_wrap(model, bool(g["guided"])), shape, clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
    return out.cpu().numpy(), model


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", sorted(LOOPS))
def test_mlp_sampling_loop_goldens(name, precision):
    g = _golden(name)
    cfg, sd, y, tape = fixture_inputs(g, loop=True)
    if LOOPS[name][5]:
        mask, target = inpaint_inputs(cfg, int(g["B"]))
        y = dict(y, inpainting_mask=mask, inpainted_motion=target)
    out, model = _loop(g, cfg, sd, y, tape, precision)
    f16, tail = model._engine.precision_plan(int(g["B"]), bool(g["guided"]))
    _close(model)
    err = float(np.abs(out - g["final"]).max())
    print(f"\n[mlp loop err] {name} {precision}: {err:.2e}")
    assert f16 == 0 and (precision == "f32" or tail == int(g["S"])), (f16, tail)      # split-bf16 on every step by default, never an fp16 sub-phase
    assert err < TOL[precision], (name, precision, err)


# ---- independence: what a tolerance hides (in-place and indexing mistakes)
def _ntu(B, seed=1):
    cfg = synth.get_config("ntu_mlp")
    sd = synth.make_state_dict(cfg, seed=0)
    return cfg, sd, {"cmotion": synth.make_cmotion(cfg, B, seed=seed)}


@pytest.mark.parametrize("precision", ["f32", "bf16_x3tail"])
def test_rows_of_a_batch_equal_single_sample_calls_bit_for_bit(precision):
    B, S = 5, 10
    cfg, sd, y = _ntu(B)
    x = synth.make_noise_tape(cfg, B, 0, seed=11)[0]
    tape = synth.make_noise_tape(cfg, B, S, seed=10)
    model, diffusion = build_hip(cfg, sd, resp=str(S), precision=precision)
    t = torch.full((B,), 400, dtype=torch.long, device="cuda")
    full = model(torch.from_numpy(x).cuda(), t, y=y_to_device(y)).cpu().numpy()
    loop = diffusion.p_sample_loop(model, x.shape, clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape)).cpu().numpy()
    for b in range(B):
        yb = y_to_device({"cmotion": y["cmotion"][b:b + 1]})
        one = model(torch.from_numpy(x[b:b + 1]).cuda(), t[:1], y=yb).cpu().numpy()
        assert np.array_equal(one[0], full[b]), ("forward", b)
        one = diffusion.p_sample_loop(model, x[b:b + 1].shape, clip_denoised=False, model_kwargs={"y": yb},
                                      noise_tape=torch.from_numpy(np.ascontiguousarray(tape[:, b:b + 1]))).cpu().numpy()
        assert np.array_equal(one[0], loop[b]), ("loop", b)
    _close(model)


def test_ragged_chains_equal_one_chain_bit_for_bit():
    """B = 7 over four kernel chains (2 + 2 + 2 + 1 samples) against one chain."""
    B, S = 7, 10
    cfg, sd, y = _ntu(B)
    tape = synth.make_noise_tape(cfg, B, S, seed=10)
    outs = {}
    for streams in (4, 1):
        model, diffusion = build_hip(cfg, sd, resp=str(S), precision="bf16_x3tail", engine_options={"STREAMS": streams})
        outs[streams] = diffusion.p_sample_loop(model, tape.shape[1:], clip_denoised=False, model_kwargs={"y": y_to_device(y)},
                                                noise_tape=torch.from_numpy(tape)).cpu().numpy()
        _close(model)
    assert np.array_equal(outs[4], outs[1])


def test_graph_replay_equals_eager_launches_bit_for_bit():
    B, S = 3, 10
    cfg = synth.get_config("tiny_mlp")
    sd = synth.make_state_dict(cfg, seed=0)
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=1), "action": synth.make_actions(cfg, B, seed=2), "scale": np.full((B,), 2.5, dtype=np.float32)}
    tape = synth.make_noise_tape(cfg, B, S, seed=10)
    model, diffusion = build_hip(cfg, sd, resp=str(S), precision="bf16_x3tail")
    outs = [diffusion.p_sample_loop(_wrap(model, True), tape.shape[1:], clip_denoised=False, model_kwargs={"y": y_to_device(y)},
                                    noise_tape=torch.from_numpy(tape), use_graph=g).cpu().numpy() for g in (True, False)]
    _close(model)
    assert np.array_equal(outs[0], outs[1])


# ---- the plain phase
def test_plain_phase_runs_the_plain_instantiations():
    """x3_tail = 0 (all plain) and 5 on mlp_ntu_ddpm50: the plain instantiation runs, the results are finite, no fp16 sub-phase. No error bound is
    asserted for the all-plain loop - the default never runs it; its error against the f32 mode is printed (profiles/mlp_arch_parity.txt)."""
    g = _golden("mlp_ntu_ddpm50")
    cfg, sd, y, tape = fixture_inputs(g, loop=True)
    outs = {}
    for tag, prec, tail in (("f32", "f32", None), ("tail0", "bf16_x3tail", 0), ("tail5", "bf16_x3tail", 5)):
        outs[tag], model = _loop(g, cfg, sd, y, tape, prec, x3_tail=tail)
        assert np.isfinite(outs[tag]).all(), tag
        if tag != "f32":
            f16, t = model._engine.precision_plan(int(g["B"]), False)
            assert (f16, t) == (0, tail), (tag, f16, t)
            plain = model._engine.plan_query(int(g["B"]), split_phase=False)
            split = model._engine.plan_query(int(g["B"]), split_phase=True)
            assert plain["mixer"]["kernel"] == "k_mix_time<bf16>" and split["mixer"]["kernel"] == "k_mix_time<bf16x3>", (plain, split)
            assert "k_layers" not in " ".join(v["kernel"] for v in plain.values()) and "k_step" not in " ".join(v["kernel"] for v in plain.values())
        _close(model)
    errs = {t: float(np.abs(outs[t] - outs["f32"]).max()) for t in ("tail0", "tail5")}
    print(f"\n[mlp plain phase vs f32 mode] mlp_ntu_ddpm50: {errs}; f32 vs reference {float(np.abs(outs['f32'] - g['final']).max()):.2e}")


# ---- refusals
def _engine(cfg, sd=None, drop=(), reshape=None, options=None, finalize=True):
    model, _ = build_hip(cfg, sd or synth.make_state_dict(cfg, seed=0))
    eng = _lib.Engine(model.engine_config(), 2, 0, "f32", **({"options": options} if options else {}))
    try:
        for k, v in (sd or synth.make_state_dict(cfg, seed=0)).items():
            if k in drop:
                continue
            eng.load_weight(k, reshape[k] if reshape and k in reshape else v)
        if finalize:
            eng.finalize()
    finally:
        eng.close()


def test_refuses_more_than_160_frames_at_create():
    cfg = synth.get_config("tiny_mlp", num_frames=161)
    with pytest.raises(_lib.RgnError, match=r"UNSUPPORTED.*160 frames"):
        _engine(cfg)
    _engine(synth.get_config("tiny_mlp", num_frames=160, layers=1))                 # ... and 160 is accepted


def test_refuses_a_layers_option():
    with pytest.raises(_lib.RgnError, match=r"UNSUPPORTED.*LAYERS.*arch='mlp'"):
        _engine(synth.get_config("tiny_mlp"), options={"LAYERS": 1})


def test_small_batch_engine_is_refused_and_reported_off():
    cfg = synth.get_config("ntu_mlp", layers=1)
    model, _ = build_hip(cfg, synth.make_state_dict(cfg, seed=0), precision="bf16_x3tail")
    x = torch.from_numpy(synth.make_noise_tape(cfg, 1, 0, seed=11)[0]).cuda()
    model(x, torch.zeros(1, dtype=torch.long, device="cuda"), y=y_to_device({"cmotion": synth.make_cmotion(cfg, 1, seed=1)}))
    eng = model._engine
    assert "sb_gemm" not in eng.plan_query(1) and "mixer" in eng.plan_query(1)          # 60 token rows: where a transformer handle takes it
    eng.set_small_batch_rows(0)
    eng.set_small_batch_rows(-1)
    with pytest.raises(_lib.RgnError, match=r"UNSUPPORTED.*small-batch.*arch='mlp'"):
        eng.set_small_batch_rows(640)
    _close(model)


def test_refuses_a_wrong_fc0_shape():
    cfg = synth.get_config("tiny_mlp")
    sd = synth.make_state_dict(cfg, seed=0)
    k = "mlp.motion_mlp.mlps.1.fc0.weight"
    with pytest.raises(_lib.RgnError, match=r"BAD_SHAPE.*fc0"):
        _engine(cfg, reshape={k: sd[k][:, :, 0]})                                   # [T, T] where the reference holds [T, T, 1]


def test_refuses_a_missing_emb_fc_key():
    with pytest.raises(_lib.RgnError, match=r"MISSING_KEY.*mlps\.1\.emb_fc\.bias"):
        _engine(synth.get_config("tiny_mlp"), drop=("mlp.motion_mlp.mlps.1.emb_fc.bias",))


def test_frame_count_other_than_num_frames_raises():
    cfg = synth.get_config("tiny_mlp")
    model, _ = build_hip(cfg, synth.make_state_dict(cfg, seed=0))
    x = torch.zeros(1, cfg["njoints"], cfg["nfeats"], cfg["num_frames"] - 1, device="cuda")
    with pytest.raises(ValueError, match="fc0"):
        model(x, torch.zeros(1, dtype=torch.long, device="cuda"), y={"cmotion": x, "action": torch.zeros(1, 1, dtype=torch.long, device="cuda")})


# ---- scoring: training_losses and calc_bpd_loop reach the model through rgn_denoise
class _Ref:
    """Stands where DistributedDataParallel stands (`.module`: the engine's owner) and answers with the fp32 restatement (+ a fixed offset)."""

    def __init__(self, module, sd, cfg, shift=None):
        self.module, self.sd, self.cfg, self.shift, self.calls = module, sd, cfg, shift, []

    def __call__(self, x, ts, y=None, **kw):
        yc = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in y.items()}
        out = mlp_arch_ref.cmdm_forward(self.sd, self.cfg, x.cpu(), ts.cpu(), yc)
        if self.shift is not None:
            out = out + self.shift[0][: out.shape[0]]
        out = out.to(x.device)
        self.calls.append(out)
        return out


class _Spy:
    def __init__(self, module):
        self.module, self.calls = module, []

    def __call__(self, x, ts, **kw):
        out = self.module(x, ts, **kw)
        self.calls.append(out.clone())
        return out


def _signs(shape, k):
    rng = np.random.Generator(np.random.PCG64(17 + k))
    return torch.from_numpy((1e-3 * rng.choice([-1.0, 1.0], shape)).astype(np.float32))


def _within_sensitivity(label, dev, ref, moved):
    """|device term - restatement term| <= the largest change of that term when the restatement's output moves by +-1e-3 (three sign patterns,
    the rule of tests/golden/make_golden_losses.py and make_golden_bpd.py) + 4 fp32 spacings."""
    for k in ref:
        a, r = dev[k].double().cpu().numpy(), ref[k].double().cpu().numpy()
        sens = np.max([np.abs(m[k].double().cpu().numpy() - r) for m in moved], axis=0)
        bound = sens + 4 * np.spacing(np.abs(r).astype(np.float32)).astype(np.float64)
        ok = np.isnan(r) | (np.abs(a - r) <= bound)
        print(f"{label} {k}: worst |dev - ref| / bound = {float(np.nanmax(np.abs(a - r) / bound)):.3f}")
        assert ok.all(), (label, k, a, r, bound)


def test_training_losses_against_the_restatement_as_the_model():
    from tests import loss_cases
    cfg = synth.get_config("tiny_mlp", njoints=56)
    sd = synth.make_state_dict(cfg, seed=0)
    B, T, thr = 3, cfg["num_frames"], 0.03
    model, diffusion = build_hip(cfg, sd)
    for k, v in dict(lambda_rcxyz=1.0, lambda_vel=1.0, lambda_fc=1.0, lambda_orient=1.0, lambda_body=1.0, lambda_transl=1.0, vel_threshold=thr,
                     num_person=1, body_model="smplx", data_rep="rot6d").items():
        setattr(diffusion, k, v)
    model.set_skeleton(synth.make_skeleton())
    try:
        inp, _, _ = loss_cases.find_inputs(B, T, "tree55", 0.01, thr, 7, max_undecided=0)
        mask = loss_cases.make_mask("ragged", B, T, 3)
        y = {"mask": torch.from_numpy(mask).reshape(B, 1, 1, T), "cmotion": torch.from_numpy(inp["cmotion"]).cuda(),
             "action": torch.from_numpy(synth.make_actions(cfg, B)).cuda()}
        t = torch.tensor([100, 500, 999], device="cuda")
        noise = torch.from_numpy(np.random.Generator(np.random.PCG64(17)).standard_normal(inp["target"].shape).astype(np.float32)).cuda()
        run = lambda m: diffusion.training_losses(m, torch.from_numpy(inp["target"]).cuda(), t, model_kwargs={"y": y}, noise=noise, dataset="ntu")
        spy, ref = _Spy(model), _Ref(model, sd, cfg)
        dev, want = run(spy), run(ref)
        err = float((spy.calls[0] - ref.calls[0]).abs().max())
        print(f"training_losses tiny_mlp: max |device model output - restatement's| = {err:.3e}")
        assert err < 1e-3, err
        moved = [run(_Ref(model, sd, cfg, shift=[_signs(inp["target"].shape, k)])) for k in range(3)]
        _within_sensitivity("training_losses", dev, want, moved)
    finally:
        model.set_skeleton(None)
        _close(model)


def test_calc_bpd_loop_against_the_restatement_as_the_model():
    from tests import bpd_ref
    cfg = synth.get_config("tiny_mlp")
    sd = synth.make_state_dict(cfg, seed=0)
    B = 2
    model, diffusion = build_hip(cfg, sd, resp="10")
    S = diffusion.num_timesteps
    try:
        x0 = torch.from_numpy(synth.make_cmotion(cfg, B, seed=4)).cuda()
        y = {"cmotion": torch.from_numpy(synth.make_cmotion(cfg, B, seed=1)).cuda(), "action": torch.from_numpy(synth.make_actions(cfg, B, seed=2)).cuda()}
        tape = torch.from_numpy(bpd_ref.noise_tape(S, B, tuple(x0.shape[1:]), 5))
        run = lambda m: diffusion.calc_bpd_loop(m, x0, clip_denoised=True, model_kwargs={"y": y}, noise_tape=tape)
        spy, ref = _Spy(model), _Ref(model, sd, cfg)
        dev, want = run(spy), run(ref)
        assert len(spy.calls) == len(ref.calls)
        err = max(float((a - b).abs().max()) for a, b in zip(spy.calls, ref.calls))
        print(f"calc_bpd_loop tiny_mlp: max |device model output - restatement's| = {err:.3e}")
        assert err < 1e-3, err
        rows = ref.calls[0].shape
        moved = [run(_Ref(model, sd, cfg, shift=[_signs(rows, k)])) for k in range(3)]
        _within_sensitivity("calc_bpd_loop", dev, want, moved)
        assert torch.equal(dev["total_bpd"], dev["vb"].sum(dim=1) + dev["prior_bpd"])
    finally:
        _close(model)
