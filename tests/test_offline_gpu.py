"""GPU: arch='offline' (the non-causal encoder denoiser, model/cmdm.py:228-238) against goldens recorded from the reference
(tests/golden/make_golden_offline.py) and against the fp32 CPU restatement tests/offline_ref.py, in every precision mode and on
every kernel form an offline handle can select."""
import os

import numpy as np
import pytest
import torch

from oracle import regennet_oracle as orc
from regennet_amd import synth
from tests import offline_ref
from tests.helpers import autoreg_inputs, build_hip, fixture_inputs, y_to_device

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PRECISIONS = ["f32", "bf16x3", "bf16_x3tail", "bf16_x3tail/throughput", "bf16x3/throughput"]
TOL = {"f32": 2e-4, "bf16x3": 1e-3, "bf16_x3tail": 1e-3, "bf16_x3tail/throughput": 1e-3, "bf16x3/throughput": 1e-3}


def _golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _wrap(model, guided):
    if not guided:
        return model
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    return ClassifierFreeSampleModel(model)


def _forward_err(g, precision, engine_options=None):
    cfg, sd, y, x = fixture_inputs(g, loop=False)
    model, _ = build_hip(cfg, sd, precision=precision, engine_options=engine_options)
    fm = _wrap(model, bool(g["guided"]))
    yd, xd = y_to_device(y), torch.from_numpy(x).cuda()
    B = x.shape[0]
    err = 0.0
    for i, t in enumerate(g["ts"]):
        out = fm(xd, torch.full((B,), int(t), dtype=torch.long, device="cuda"), y=yd)
        err = max(err, float(np.abs(out.cpu().numpy() - g["out"][i]).max()))
    for i, t in enumerate(g.get("uncond_ts", [])):
        out = model(xd, torch.full((B,), int(t), dtype=torch.long, device="cuda"), y=dict(yd, uncond=True))
        err = max(err, float(np.abs(out.cpu().numpy() - g["out_uncond"][i]).max()))
    return err, model


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["offline_tiny_fwd", "offline_tiny_fwd_cfg", "offline_ntu_fwd", "offline_chi3d_fwd"])
def test_offline_forward_goldens(name, precision):
    if "/" in precision and "tiny" in name:
        pytest.skip("the small-batch engine only takes d = 512 models: same kernels as the plain mode")
    err, _ = _forward_err(_golden(name), precision)
    assert err < TOL[precision], (name, precision, err)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["offline_tiny_add_ddpm10", "offline_tiny_ddim10_cfg", "offline_ntu_ddpm50", "offline_chi3d_ddim20_cfg"])
def test_offline_sampling_loop_goldens(name, precision):
    if "/" in precision and "tiny" in name:
        pytest.skip("the small-batch engine only takes d = 512 models: same kernels as the plain mode")
    g = _golden(name)
    cfg, sd, y, tape = fixture_inputs(g, loop=True)
    model, diffusion = build_hip(cfg, sd, resp=str(g["resp"]), precision=precision)
    fm = _wrap(model, bool(g["guided"]))
    shape = (int(g["B"]), cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    fn = diffusion.p_sample_loop if str(g["mode"]) == "ddpm" else diffusion.ddim_sample_loop
    out = fn(fm, shape, clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
    err = float(np.abs(out.cpu().numpy() - g["final"]).max())
    print(f"\n[offline loop err] {name} {precision}: {err:.2e}")
    assert err < TOL[precision], (name, precision, err)


@pytest.mark.parametrize("name,precision,opts", [
    ("offline_ntu_fwd", "bf16x3/throughput", {"QKV_X3_DMA": 1}),        # k_qkv_attn<full> (direct-to-LDS split form)
    ("offline_ntu_fwd", "bf16x3/throughput", {"MLP_X3": 0}),            # k_gemm_x3 + k_layernorm tail, one norm
])
def test_offline_switch_forms(name, precision, opts):
    err, _ = _forward_err(_golden(name), precision, engine_options=opts)
    assert err < 1e-3, (name, opts, err)


def test_offline_plain_phase_forms_at_61_and_151_tokens():
    """The plain phase of the precision schedule, which offline handles run only where x3_tail is set (the default tail is every step):
    k_qkv_attn_rs<full> + k_mlp2<enc> at 61 tokens, k_rowgemm in_proj + k_attn_x3<full> + k_mlp2<enc> at 151. Reports the loop error of
    tail 0 (all plain) and tail 5 against the fp32 mode; asserts the forms and finite results."""
    errs = {}
    for name in ("offline_ntu_ddpm50", "offline_chi3d_ddim20_cfg"):
        g = _golden(name)
        cfg, sd, y, tape = fixture_inputs(g, loop=True)
        shape = (int(g["B"]), cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
        kw = dict(clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
        outs = {}
        for tag, prec, tail in (("f32", "f32", None), ("tail0", "bf16_x3tail/throughput", 0), ("tail5", "bf16_x3tail/throughput", 5)):
            model, diffusion = build_hip(cfg, sd, resp=str(g["resp"]), precision=prec, x3_tail=tail)
            fn = diffusion.p_sample_loop if str(g["mode"]) == "ddpm" else diffusion.ddim_sample_loop
            outs[tag] = fn(_wrap(model, bool(g["guided"])), shape, **kw).cpu().numpy()
            assert np.isfinite(outs[tag]).all(), (name, tag)
            if tag == "tail0":
                plan = model._engine.plan_query(int(g["B"]), guided=bool(g["guided"]), split_phase=False)
                kinds = {v["kernel"] for v in plan.values()}
                assert "k_mlp2<enc>" in kinds, plan
                assert ("k_qkv_attn_rs<full>" in kinds) if cfg["num_frames"] == 60 else ("k_attn_x3<full>" in kinds and "rowgemm_act" in plan), plan
        errs[name] = {t: float(np.abs(outs[t] - outs["f32"]).max()) for t in ("tail0", "tail5")}
        errs[name]["f32_vs_reference"] = float(np.abs(outs["f32"] - g["final"]).max())
    # the online emb_trans_dec model of the NTU shapes on the same loop (its causal twin; the 8-layer decoder without the embedding token
    # is what the online schedule tests bound)
    cfg = synth.get_config("ntu", emb_trans_dec=True)
    sd = synth.make_state_dict(cfg, seed=0)
    g = _golden("offline_ntu_ddpm50")
    tape = synth.make_noise_tape(cfg, int(g["B"]), int(g["S"]), seed=10)
    yd = y_to_device({"cmotion": synth.make_cmotion(cfg, int(g["B"]), seed=1)})
    outs = {}
    for tag, prec, tail in (("f32", "f32", None), ("tail0", "bf16_x3tail/throughput", 0), ("tail5", "bf16_x3tail/throughput", 5)):
        model, diffusion = build_hip(cfg, sd, resp=str(g["resp"]), precision=prec, x3_tail=tail)
        outs[tag] = diffusion.p_sample_loop(model, tape.shape[1:], clip_denoised=False, model_kwargs={"y": yd}, noise_tape=torch.from_numpy(tape)).cpu().numpy()
    errs["online_etd_ntu_ddpm50"] = {t: float(np.abs(outs[t] - outs["f32"]).max()) for t in ("tail0", "tail5")}
    print(f"\n[offline plain phase vs fp32 mode] {errs}")


def _plain_eval_errs(frames):
    """One denoiser evaluation of B = 2 motions in each plain-bf16 arithmetic, against the fp32 CPU forward, for the offline model and
    for the online emb_trans_dec model of the same shapes and draws (the causal twin: same kernels but for the mask and the
    cross-attention / middle norm). 'bf16': the plain precision mode (k_qkv_attn<false> / k_gemm_x3 + k_attn_x3, k_gemm_x3 + k_layernorm
    tail). 'phase': the precision schedule's plain phase, reached through a one-step loop (timestep 0, where the sampler returns the
    prediction itself) with x3_tail = 0 on the throughput kernels: k_qkv_attn_rs + k_mlp2 at 61 tokens, k_rowgemm in_proj + k_attn_x3 +
    k_mlp2 at 151 (the online model with NO_QKV_LONG=1, its switch to the same form)."""
    B = 2
    errs = {}
    for arch in ("offline", "online_etd"):
        cfg = synth.get_config("ntu_offline" if arch == "offline" else "ntu", num_frames=frames, **({} if arch == "offline" else {"emb_trans_dec": True}))
        sd = synth.make_state_dict(cfg, seed=0)
        y = {"cmotion": synth.make_cmotion(cfg, B, seed=1)}
        x = synth.make_noise_tape(cfg, B, 0, seed=11)[0]
        yt = {k: torch.from_numpy(v) for k, v in y.items()}
        ref_fwd = offline_ref.cmdm_forward if arch == "offline" else orc.cmdm_forward
        ref = {t: ref_fwd(sd, cfg, torch.from_numpy(x), torch.full((B,), t, dtype=torch.long), yt).numpy() for t in (0, 500)}
        model, _ = build_hip(cfg, sd, precision="bf16/throughput")
        errs[(arch, "bf16")] = max(float(np.abs(model(torch.from_numpy(x).cuda(), torch.full((B,), t, device="cuda"), y=y_to_device(y)).cpu().numpy()
                                               - ref[t]).max()) for t in (0, 500))
        opts = {"NO_QKV_LONG": 1} if arch == "online_etd" else None
        model, diffusion = build_hip(cfg, sd, resp="1", precision="bf16_x3tail/throughput", x3_tail=0, engine_options=opts)
        tape = np.stack([x, np.zeros_like(x)])
        out = diffusion.p_sample_loop(model, x.shape, clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
        errs[(arch, "phase")] = float(np.abs(out.cpu().numpy() - ref[0]).max())
        kinds = {v["kernel"] for v in model._engine.plan_query(B, split_phase=False).values()}
        want = ({"k_qkv_attn_rs<full>", "k_mlp2<enc>"} if frames == 60 else {"k_attn_x3<full>", "k_mlp2<enc>"}) if arch == "offline" else \
               ({"k_qkv_attn_rs", "k_mlp2"} if frames == 60 else {"k_attn_x3", "k_mlp2"})
        assert want <= kinds, (arch, kinds)
    return errs


@pytest.mark.parametrize("frames", [60, 150])
def test_offline_plain_bf16_forms_against_reference(frames):
    """The plain-bf16 encoder forms (the precision mode 'bf16', and the schedule's plain phase that an explicit or calibrated x3_tail
    selects) on one evaluation: within the plain-bf16 error class of their causal twins on the online emb_trans_dec model (measured: offline
    3.2e-2 / 3.1e-2, online emb_trans_dec 2.9e-2 / 2.0e-2 at 61 and 151 tokens - bf16 operand rounding through 8 layers at d = 512)."""
    errs = _plain_eval_errs(frames)
    print(f"\n[plain bf16, one evaluation, {frames + 1} tokens] " + ", ".join(f"{a}/{m}: {e:.2e}" for (a, m), e in errs.items()))
    for mode in ("bf16", "phase"):
        assert errs[("offline", mode)] <= 2.0 * errs[("online_etd", mode)], (mode, errs)
        assert errs[("offline", mode)] < 5e-2, (mode, errs)


@pytest.mark.parametrize("T", [31, 32, 63, 64, 150])
def test_offline_sequence_length_edges(T):
    """Tq = T + 1 = 32, 33, 64, 65 and 151 tokens at d = 512: masking of the padding keys of every full-attention form."""
    cfg = synth.get_config("ntu_offline", num_frames=T, layers=2)
    sd = synth.make_state_dict(cfg, seed=3)
    B = 2
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=5)}
    x = synth.make_noise_tape(cfg, B, 0, seed=6)[0]
    ts = torch.tensor([5, 800])
    ref = offline_ref.cmdm_forward(sd, cfg, torch.from_numpy(x), ts, {k: torch.from_numpy(v) for k, v in y.items()}).numpy()
    for precision in ("f32", "bf16x3/throughput", "bf16x3"):
        model, _ = build_hip(cfg, sd, precision=precision)
        out = model(torch.from_numpy(x).cuda(), ts.cuda(), y=y_to_device(y)).cpu().numpy()
        err = float(np.abs(out - ref).max())
        assert err < 1e-3, (T, precision, err)


def test_non_causality_witness():
    """Change only the actor's LAST frame: offline output frame 0 moves, an online emb_trans_dec model's frame 0 does not."""
    B = 1
    outs = {}
    for arch, cfg in (("offline", synth.get_config("ntu_offline", layers=2)), ("online", synth.get_config("ntu", layers=2, emb_trans_dec=True))):
        sd = synth.make_state_dict(cfg, seed=0)
        model, _ = build_hip(cfg, sd, precision="bf16x3/throughput")
        x = torch.from_numpy(synth.make_noise_tape(cfg, B, 0, seed=11)[0]).cuda()
        cm = synth.make_cmotion(cfg, B, seed=1)
        cm2 = cm.copy()
        cm2[..., -1] += 0.5
        t = torch.tensor([300], device="cuda")
        a = model(x, t, y=y_to_device({"cmotion": cm})).cpu().numpy()
        b = model(x, t, y=y_to_device({"cmotion": cm2})).cpu().numpy()
        outs[arch] = float(np.abs(a[..., 0] - b[..., 0]).max())
    assert outs["offline"] > 1e-3, outs
    assert outs["online"] == 0.0, outs


def test_offline_rows_equal_single_sample_runs():
    """A B = 256 ntu_offline evaluation - the headline offline shape, where k_qkv_attn_rs_x3<full> runs two heads per workgroup (its
    second S^T exchange pass once per head, between the heads' barriers) - row for row equal to B = 1 runs (one head per workgroup)."""
    cfg = synth.get_config("ntu_offline")
    sd = synth.make_state_dict(cfg, seed=0)
    B = 256
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=1)}
    x = synth.make_noise_tape(cfg, B, 0, seed=11)[0]
    model, _ = build_hip(cfg, sd, precision="bf16x3/throughput")
    t = torch.full((B,), 400, dtype=torch.long, device="cuda")
    full = model(torch.from_numpy(x).cuda(), t, y=y_to_device(y)).cpu().numpy()
    assert model._engine.plan_query(B, split_phase=True)["qkv_attn"]["kernel"] == "k_qkv_attn_rs_x3<full>"
    for b in (0, 1, 127, 200, 255):
        one = model(torch.from_numpy(x[b:b + 1]).cuda(), t[:1], y=y_to_device({"cmotion": y["cmotion"][b:b + 1]})).cpu().numpy()
        assert np.array_equal(one[0], full[b]), b


@pytest.mark.parametrize("precision", ["bf16_x3tail", "bf16_x3tail/throughput"])
def test_offline_guided_b64_ddim_matches_reference(precision):
    """ntu_action_offline, B = 64, 5-step DDIM + CFG (128 evaluation rows per step) against the reference's own run (rows kept by the
    recorder: make_golden_offline.gen_loop_rows)."""
    g = _golden("offline_ntu_action_ddim5_cfg_b64")
    cfg, sd, y, tape = fixture_inputs(g, loop=True)
    model, diffusion = build_hip(cfg, sd, resp=str(g["resp"]), precision=precision)
    shape = (int(g["B"]), cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    out = diffusion.ddim_sample_loop(_wrap(model, True), shape, clip_denoised=False, model_kwargs={"y": y_to_device(y)},
                                     noise_tape=torch.from_numpy(tape)).cpu().numpy()
    err = float(np.abs(out[g["rows"]] - g["final_rows"]).max())
    print(f"\n[offline guided B=64] {precision}: {err:.2e}")
    assert err < 1e-3, (precision, err)


def test_offline_plan_names_the_full_and_encoder_instantiations():
    cfg = synth.get_config("ntu_offline")
    sd = synth.make_state_dict(cfg, seed=0)
    model, diffusion = build_hip(cfg, sd, resp="10", precision="bf16_x3tail/throughput")
    y = {"cmotion": synth.make_cmotion(cfg, 64, seed=1)}
    x = torch.from_numpy(synth.make_noise_tape(cfg, 64, 0, seed=11)[0]).cuda()
    model(x, torch.full((64,), 5, dtype=torch.long, device="cuda"), y=y_to_device(y))
    eng = model._engine
    split = eng.plan_query(64, split_phase=True)
    plain = eng.plan_query(64, split_phase=False)
    assert split["qkv_attn"]["kernel"] == "k_qkv_attn_rs_x3<full>" and split["mlp"]["kernel"] == "k_mlp_x3<enc>", split
    assert plain["qkv_attn"]["kernel"] == "k_qkv_attn_rs<full>" and plain["mlp"]["kernel"] == "k_mlp2<enc>", plain
    for plan in (split, plain):
        kinds = " ".join(v["kernel"] for v in plan.values())
        assert "k_layers" not in kinds and "k_step" not in kinds and "k_qkv_attn_long" not in kinds, plan
    model, diffusion = build_hip(cfg, sd, resp="10", precision="f32")      # (61 tokens, heads of 128: the MFMA tiles, full form)
    model(x, torch.full((64,), 5, dtype=torch.long, device="cuda"), y=y_to_device(y))
    f32 = model._engine.plan_query(64, split_phase=True)
    assert f32["attention"]["kernel"] == "k_attn_mfma<full>" and f32["gemm_mfma"]["kernel"] == "k_gemm_f32", f32


def test_offline_auto_regressive_matches_reference_frame_loop():
    from regennet_amd.eval import sample_auto_regressive
    g = _golden("offline_tiny_add_autoreg_ddpm10")
    cfg, sd, y, tapes = autoreg_inputs(g)
    model, diffusion = build_hip(cfg, sd, resp=str(g["resp"]), precision="bf16x3")
    B, T = int(g["B"]), int(g["T"])
    out = sample_auto_regressive(diffusion.p_sample_loop, model, (B, cfg["njoints"], cfg["nfeats"], T), {"y": y_to_device(y)},
                                 frames_per_call=3, noise_tapes=[torch.from_numpy(t) for t in tapes])
    err = float(np.abs(out.cpu().numpy() - g["output"]).max())
    assert err < 1e-3, err
