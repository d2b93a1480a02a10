"""GPU: the HIP path (through the C-ABI) against golden vectors recorded from the reference and against
the oracle on the same seeded inputs. Tolerance from BASELINE.json north_star: 1e-3 abs on rot6d
(written per test); timestep indices bit-exact."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import autoreg_inputs, build_hip, fixture_inputs, fixture_opts, y_to_device

pytestmark = pytest.mark.gpu

# "<mode>/throughput" (tests/helpers.py build_hip): small-batch engine off, i.e. the kernels of a full-size batch. Without
# it, evaluations of <= 640 token rows of a d = 512 model (every d = 512 golden here) run the column-split small-batch
# kernels (rgn_sb.hip).
PRECISIONS = ["f32", "bf16x3", "bf16_x3tail", "bf16_x3tail/throughput", "bf16x3/throughput"]
# abs; all inside the 1e-3 contract. "bf16_x3tail" (the default) = the precision schedule: plain-bf16 GEMM operands for
# the bulk of a sampling loop, split-bf16 for its last steps and for single evaluations.
TOL = {"f32": 2e-4, "bf16x3": 1e-3, "bf16_x3tail": 1e-3, "bf16_x3tail/throughput": 1e-3, "bf16x3/throughput": 1e-3}


def _skip_redundant(name, precision):
    if "/" in precision and name.startswith("tiny"):
        pytest.skip("the small-batch engine only takes d = 512 models: same kernels as the plain mode")

FWD = ["tiny_fwd", "tiny_fwd_cfg", "tiny_add_fwd", "tiny_etd_fwd", "tiny_wope_fwd", "tiny_text_fwd_cfg", "ntu_fwd",
       "ntu_action_fwd_cfg", "chi3d_fwd"]
LOOPS = ["tiny_ddpm10", "tiny_ddim10_cfg", "tiny_add_ddpm1000", "tiny_text_ddim20_cfg", "tiny_etd_ddim10_cfg",
         "tiny_wope_ddpm10", "ntu_add_etd_ddpm20", "ntu_ddpm50",
         "ntu_action_ddim100_cfg", "text150_ddim50_cfg", "chi3d_ddpm20", "chi3d_ddim20_cfg"]


def default_tail(S, layers=8):
    """rgn_plan.cpp default_tail(): loop indices below this run split-bf16 under the precision schedule."""
    from regennet_amd._lib import default_x3_tail
    return default_x3_tail(S, layers)


def _wrap(model, guided):
    if not guided:
        return model
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    return ClassifierFreeSampleModel(model)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", FWD)
def test_denoiser_forward(golden, name, precision):
    _skip_redundant(name, precision)
    g = golden(name)
    cfg, sd, y, x = fixture_inputs(g, loop=False)
    model, _ = build_hip(cfg, sd, precision=precision)
    fm = _wrap(model, bool(g["guided"]))
    yd = y_to_device(y)
    xd = torch.from_numpy(x).cuda()
    for i, t in enumerate(g["ts"]):
        out = fm(xd, torch.full((x.shape[0],), int(t), dtype=torch.long, device="cuda"), y=yd)
        assert out.shape == xd.shape and out.dtype == torch.float32 and out.is_cuda
        err = np.abs(out.cpu().numpy() - g["out"][i]).max()
        assert err < TOL[precision], (name, int(t), err)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", LOOPS)
def test_sampling_loop(golden, name, precision):
    _skip_redundant(name, precision)
    g = golden(name)
    cfg, sd, y, tape = fixture_inputs(g, loop=True)
    model, diffusion = build_hip(cfg, sd, resp=str(g["resp"]), precision=precision)
    # bit-exact timestep indices (respace.py:124-129)
    step = 2 if bool(g["guided"]) else 1
    assert diffusion.timestep_map[::-1] == g["model_t"][::step].tolist()
    fm = _wrap(model, bool(g["guided"]))
    shape = (int(g["B"]), cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    fn = diffusion.p_sample_loop if str(g["mode"]) == "ddpm" else diffusion.ddim_sample_loop
    out = fn(fm, shape, clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
    err = np.abs(out.cpu().numpy() - g["final"]).max()
    print(f"\n[loop err] {name} {precision}: {err:.2e}")
    assert err < TOL[precision], (name, err)
    if "x0" in g:   # per-step trace through the progressive API
        pfn = diffusion.p_sample_loop_progressive if str(g["mode"]) == "ddpm" else diffusion.ddim_sample_loop_progressive
        S = int(g["S"])
        for k, o in enumerate(pfn(fm, shape, clip_denoised=False, model_kwargs={"y": y_to_device(y)},
                                  noise_tape=torch.from_numpy(tape))):
            # (under the default precision schedule the progressive generators run split-bf16 throughout, so every yielded
            # state is inside the bound, not only the last)
            assert np.abs(o["pred_xstart"].cpu().numpy() - g["x0"][k]).max() < TOL[precision]
            assert np.abs(o["sample"].cpu().numpy() - g["x"][k]).max() < TOL[precision]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_headline_1000_step_ddpm(golden, precision):
    """BASELINE configs[0]/[1] shape: NTU120-AS, 1000-step DDPM, identical noise; <= 1e-3 abs vs the reference."""
    g = golden("ntu_ddpm1000")
    cfg, sd, y, tape = fixture_inputs(g, loop=True)
    model, diffusion = build_hip(cfg, sd, precision=precision)
    assert diffusion.timestep_map == list(range(1000)) and g["model_t"].tolist() == list(range(999, -1, -1))
    shape = (2, 56, 6, 60)
    out = diffusion.p_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": y_to_device(y)},
                                  noise_tape=torch.from_numpy(tape), use_graph=True)
    err = np.abs(out.cpu().numpy() - g["final"]).max()
    assert err < TOL[precision], err


@pytest.mark.parametrize("engine", ["throughput", "small-batch"])
@pytest.mark.parametrize("name", ["ntu_ddpm1000", "ntu_action_ddim100_cfg", "text150_ddim50_cfg", "chi3d_ddim20_cfg"])
def test_precision_schedule_switch_point_sweep(golden, name, engine):
    """Precision schedule (RGN_PREC_BF16_X3TAIL): plain-bf16 GEMMs for loop indices >= tail, split-bf16 below. Early-step
    error is contracted by the sampler (posterior_mean_coef1 -> 0 at large t, gaussian_diffusion.py:265-276), so a short
    split-bf16 tail recovers the parity bound. Sweeps the switch point against the reference's 1000-step DDPM and guided
    100-step DDIM outputs (and the 150-frame goldens: in "throughput" mode their plain-bf16 steps run the fused long-sequence
    in_proj + attention kernel, k_qkv_attn_long): the default and every tail >= 5 must meet 1e-3; all-bf16 (tail 0) is reported, not asserted."""
    g = golden(name)
    cfg, sd, y, tape = fixture_inputs(g, loop=True)
    S = int(g["S"])
    errs = {}
    shape = (int(g["B"]), cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    for tail in (0, 2, 3, 5, 10, 25, None, S):
        model, diffusion = build_hip(cfg, sd, resp=str(g["resp"]), precision="bf16_x3tail/" + engine, x3_tail=tail)
        fm = _wrap(model, bool(g["guided"]))
        fn = diffusion.p_sample_loop if str(g["mode"]) == "ddpm" else diffusion.ddim_sample_loop
        out = fn(fm, shape, clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
        errs[tail] = float(np.abs(out.cpu().numpy() - g["final"]).max())
        model._engine.close()
    print(f"\n[x3-tail sweep] {name} {engine} (default tail {default_tail(S, cfg['layers'])}): " + ", ".join(f"{k}: {v:.2e}" for k, v in errs.items()))
    for tail, e in errs.items():
        if tail is None or tail >= 5:
            assert e < 1e-3, (name, tail, e)
    assert errs[None] < 3.5e-4, errs        # the default keeps a 3x margin on these goldens
    # tail = S is the uniform split-bf16 mode
    model, diffusion = build_hip(cfg, sd, resp=str(g["resp"]), precision="bf16x3/" + engine)
    fm = _wrap(model, bool(g["guided"]))
    fn = diffusion.p_sample_loop if str(g["mode"]) == "ddpm" else diffusion.ddim_sample_loop
    ref = fn(fm, shape, clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
    assert abs(float(np.abs(ref.cpu().numpy() - g["final"]).max()) - errs[S]) < 1e-6


@pytest.mark.parametrize("precision", PRECISIONS)
def test_graph_replay_equals_eager(golden, precision):
    g = golden("ntu_ddpm50")
    cfg, sd, y, tape = fixture_inputs(g, loop=True)
    model, diffusion = build_hip(cfg, sd, resp="50", precision=precision)
    shape = (2, 56, 6, 60)
    kw = dict(clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
    a = diffusion.p_sample_loop(model, shape, use_graph=False, **kw)
    b = diffusion.p_sample_loop(model, shape, use_graph=True, **kw)
    c = diffusion.p_sample_loop(model, shape, use_graph=True, **kw)   # replays the cached graph
    assert torch.equal(a, b) and torch.equal(b, c)


@pytest.mark.parametrize("engine", ["throughput", "small-batch"])
def test_the_phase_of_an_evaluation_does_not_leak_between_calls(engine):
    """The arithmetic of an evaluation (split-bf16 | plain, fp16 operands) is an argument of the dispatch, not state a call leaves behind on
    the handle: rgn_denoise is always split-bf16 under the precision schedule, so after an eager sampling loop and after a graph-replayed one
    (10-step DDPM, 8 plain + 2 split steps) it must return, bit for bit, what a fresh engine that never sampled returns; and the two loops
    must agree bit for bit on the same noise tape."""
    from regennet_amd import synth
    cfg = synth.get_config("tiny")
    sd = synth.make_state_dict(cfg, seed=0)
    B = 2
    shape = (B, cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    y = y_to_device({"cmotion": synth.make_cmotion(cfg, B), "action": synth.make_actions(cfg, B)})
    x = torch.from_numpy(synth.make_noise_tape(cfg, B, 1, seed=3)[0]).cuda()
    t = torch.tensor([7, 2], dtype=torch.long, device="cuda")
    kw = dict(clip_denoised=False, model_kwargs={"y": y}, noise_tape=torch.from_numpy(synth.make_noise_tape(cfg, B, 10, seed=10)))
    build = lambda: build_hip(cfg, sd, resp="10", precision="bf16_x3tail/" + engine, x3_tail=2)
    fresh, _ = build()
    want = fresh(x, t, y=y).clone()
    model, diffusion = build()
    eager = diffusion.p_sample_loop(model, shape, use_graph=False, **kw).clone()
    after_eager = model(x, t, y=y).clone()
    replay = diffusion.p_sample_loop(model, shape, use_graph=True, **kw).clone()
    after_replay = model(x, t, y=y).clone()
    assert torch.equal(after_eager, want) and torch.equal(after_replay, want)
    assert torch.equal(eager, replay)


def test_precision_schedule_auto_calibration_and_conservative_defaults():
    """The schedule's validity depends on how strongly a checkpoint damps early-step rounding (depth, emb_trans_dec,
    guidance: DESIGN.md §6). (1) `x3_tail="auto"` measures it on the checkpoint itself: a shallow guided model gets a longer
    split-bf16 tail than the depth-scaled default would need to be trusted blindly, and ends inside the parity bound;
    (2) emb_trans_dec models default to split-bf16 throughout (bit-identical to the uniform mode)."""
    from oracle import regennet_oracle as orc
    from regennet_amd import synth
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    cfg = synth.get_config("ntu_action", layers=2)
    sd = synth.make_state_dict(cfg, seed=5)
    B = 2
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=61), "action": synth.make_actions(cfg, B, seed=62), "scale": np.full((B,), 2.5, np.float32)}
    tape = synth.make_noise_tape(cfg, B, 100, seed=63)
    ref = orc.sample_loop(sd, cfg, orc.make_schedule("cosine", "ddim100"), tape, {k: torch.from_numpy(v) for k, v in y.items()},
                          mode="ddim", guided=True).numpy()
    model, diffusion = build_hip(cfg, sd, resp="ddim100", precision="bf16_x3tail", x3_tail="auto")
    fm = ClassifierFreeSampleModel(model)
    out = diffusion.ddim_sample_loop(fm, (B, 56, 6, 60), clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
    chosen = model._auto_tail
    err = float(np.abs(out.cpu().numpy() - ref).max())
    print(f"\n[auto tail] 2 layers, ddim100 + CFG: chose {chosen} of 100, error vs oracle {err:.2e}")
    assert 8 <= chosen <= 100 and err < 1e-3
    again = diffusion.ddim_sample_loop(fm, (B, 56, 6, 60), clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
    assert torch.equal(out, again) and model._auto_tail == chosen            # calibrated once, cached per (schedule, sampler, guidance, T)
    # emb_trans_dec: default = uniform split-bf16
    cfg2 = synth.get_config("ntu_action", layers=2, emb_trans_dec=True)
    sd2 = synth.make_state_dict(cfg2, seed=5)
    tape2 = torch.from_numpy(synth.make_noise_tape(cfg2, B, 50, seed=63))
    outs = []
    for prec in ("bf16_x3tail", "bf16x3"):
        m2, d2 = build_hip(cfg2, sd2, resp="ddim50", precision=prec)
        outs.append(d2.ddim_sample_loop(ClassifierFreeSampleModel(m2), (B, 56, 6, 60), clip_denoised=False, model_kwargs={"y": y_to_device(y)},
                                        noise_tape=tape2))
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("engine", ["throughput", "small-batch"])
def test_multi_step_graphs_equal_single_step_replay(golden, monkeypatch, engine):
    """rgn_sample_range replays graphs that hold several loop iterations each (the loop index lives on the device): 1, 7
    or 10 iterations per graph, or eager launches, must not change a bit — across the phase switch of the schedule too."""
    g = golden("ntu_ddpm50")
    cfg, sd, y, tape = fixture_inputs(g, loop=True)
    outs = []
    for steps in ("1", "7", "10"):
        monkeypatch.setenv("REGENNET_GRAPH_STEPS", steps)
        model, diffusion = build_hip(cfg, sd, resp="50", precision="bf16_x3tail/" + engine)
        kw = dict(clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
        outs.append(diffusion.p_sample_loop(model, (2, 56, 6, 60), **kw))
        if steps == "7":
            outs.append(diffusion.p_sample_loop(model, (2, 56, 6, 60), use_graph=False, **kw))
        model._engine.close()
    for o in outs[1:]:
        assert torch.equal(outs[0], o)
    assert np.abs(outs[0].cpu().numpy() - g["final"]).max() < 1e-3


@pytest.mark.parametrize("engine", ["throughput", "small-batch"])
@pytest.mark.parametrize("frames,etd", [(16, False), (64, False), (63, True), (64, True)])
def test_oracle_parity_sequence_length_edges(frames, etd, engine):
    """The fused in_proj+attention kernel takes Tq <= 64 tokens: one token tile only (16), exactly full tiles (64, and
    63 + the emb_trans_dec token), and one token too many (64 + 1 -> the unfused GEMM + attention kernels)."""
    from oracle import regennet_oracle as orc
    from regennet_amd import synth
    cfg = synth.get_config("ntu_action", layers=2, num_frames=frames, emb_trans_dec=etd)
    sd = synth.make_state_dict(cfg, seed=9)
    B = 3
    model, diffusion = build_hip(cfg, sd, resp="ddim5", precision="bf16x3/" + engine)
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=31), "action": synth.make_actions(cfg, B, seed=32)}
    tape = synth.make_noise_tape(cfg, B, 5, seed=33)
    ty = {k: torch.from_numpy(v) for k, v in y.items()}
    ref = orc.sample_loop(sd, cfg, orc.make_schedule("cosine", "ddim5"), tape, ty, mode="ddim").numpy()
    out = diffusion.ddim_sample_loop(model, (B, 56, 6, frames), clip_denoised=False, model_kwargs={"y": y_to_device(y)},
                                     noise_tape=torch.from_numpy(tape))
    assert np.abs(out.cpu().numpy() - ref).max() < 1e-3


@pytest.mark.parametrize("frames,etd", [(65, False), (100, False), (160, False), (159, True)])
def test_oracle_parity_long_sequence_fused_attention(frames, etd):
    """k_qkv_attn_long (plain-bf16 phase, 65 .. 160 tokens: in_proj + flash-style attention per (sample, head) with q / k / v
    in LDS): the shortest and the longest sequence it takes, a length that is not a multiple of the 32-token tiles, and the
    emb_trans_dec token as the 160th; odd batch; against the oracle on a 10-step guided DDIM loop whose first 7 steps run the
    plain-bf16 phase (emb_trans_dec models default to split-bf16 throughout, so the tail is forced)."""
    from oracle import regennet_oracle as orc
    from regennet_amd import synth
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    cfg = synth.get_config("chi3d", num_frames=frames, emb_trans_dec=etd)
    sd = synth.make_state_dict(cfg, seed=11)
    B = 3
    model, diffusion = build_hip(cfg, sd, resp="ddim10", precision="bf16_x3tail/throughput", x3_tail=3)
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=71), "action": synth.make_actions(cfg, B, seed=72), "scale": np.full((B,), 2.5, np.float32)}
    tape = synth.make_noise_tape(cfg, B, 10, seed=73)
    ref = orc.sample_loop(sd, cfg, orc.make_schedule("cosine", "ddim10"), tape, {k: torch.from_numpy(v) for k, v in y.items()},
                          mode="ddim", guided=True).numpy()
    out = diffusion.ddim_sample_loop(ClassifierFreeSampleModel(model), (B, 56, 6, frames), clip_denoised=False,
                                     model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
    err = float(np.abs(out.cpu().numpy() - ref).max())
    print(f"\n[long fused attention] T={frames} etd={etd}: {err:.2e}")
    assert err < 1e-3, (frames, etd, err)


@pytest.mark.parametrize("engine", ["throughput", "small-batch"])
@pytest.mark.parametrize("over", [dict(ff_size=512), dict(ff_size=2048), dict(latent_dim=256, ff_size=1024), dict(num_frames=24, emb_trans_dec=True)])
def test_oracle_parity_across_kernel_dispatch_paths(over, engine):
    """The plain-bf16 phase picks its kernels by shape: d = 512 / ff = 1024 -> k_mlp; d = 512 with another ff -> k_rowgemm
    (ff = 512) or the generic tiles (ff = 2048: activation image too large); other widths -> generic tiles. Each path against
    the oracle under the default precision schedule (2 layers, 50 steps: 18 plain-bf16 + 32 split-bf16) and with guidance.
    engine "small-batch": the same shapes through the column-split kernels (ff % 32 == 0 from 512 on; d = 512 only)."""
    if engine == "small-batch" and over.get("latent_dim", 512) != 512:
        pytest.skip("small-batch engine: d = 512 only")
    from oracle import regennet_oracle as orc
    from regennet_amd import synth
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    cfg = synth.get_config("ntu_action", layers=2, **over)
    sd = synth.make_state_dict(cfg, seed=5)
    B, T = 3, cfg["num_frames"]
    model, diffusion = build_hip(cfg, sd, resp="ddim50", precision="bf16_x3tail/" + engine)
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=61), "action": synth.make_actions(cfg, B, seed=62), "scale": np.full((B,), 2.5, np.float32)}
    tape = synth.make_noise_tape(cfg, B, 50, seed=63)
    ref = orc.sample_loop(sd, cfg, orc.make_schedule("cosine", "ddim50"), tape, {k: torch.from_numpy(v) for k, v in y.items()},
                          mode="ddim", guided=True).numpy()
    out = diffusion.ddim_sample_loop(ClassifierFreeSampleModel(model), (B, 56, 6, T), clip_denoised=False,
                                     model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
    err = float(np.abs(out.cpu().numpy() - ref).max())
    print(f"\n[dispatch path] {over} {engine}: {err:.2e}")
    assert err < 1e-3, (over, err)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_oracle_parity_random_inputs(precision):
    """HIP vs oracle on fresh seeded inputs (not the golden ones), ragged batch (odd: the fused in_proj+attention kernel
    gets full sample pairs and a half-empty one), sequence shorter than the 64-token tile, mid-size model."""
    from oracle import regennet_oracle as orc
    from regennet_amd import synth
    cfg = synth.get_config("ntu_action", layers=3, num_frames=37)
    sd = synth.make_state_dict(cfg, seed=7)
    B = 5
    model, diffusion = build_hip(cfg, sd, resp="ddim20", precision=precision)
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=21), "action": synth.make_actions(cfg, B, seed=22)}
    tape = synth.make_noise_tape(cfg, B, 20, seed=23)
    ty = {k: torch.from_numpy(v) for k, v in y.items()}
    ref = orc.sample_loop(sd, cfg, orc.make_schedule("cosine", "ddim20"), tape, ty, mode="ddim").numpy()
    out = diffusion.ddim_sample_loop(model, (B, 56, 6, 37), clip_denoised=False, model_kwargs={"y": y_to_device(y)},
                                     noise_tape=torch.from_numpy(tape))
    assert np.abs(out.cpu().numpy() - ref).max() < 1e-3


def test_philox_stream_properties():
    """On-device N(0,1): moments, world-size invariance (sample_offset), determinism, x_T != per-step stream."""
    from regennet_amd import synth
    cfg = synth.get_config("ntu", layers=1)
    sd = synth.make_state_dict(cfg, seed=0)
    model, diffusion = build_hip(cfg, sd, resp="ddim5")
    eng, dev = model._get_engine(8)
    st = torch.cuda.current_stream().cuda_stream
    a = torch.empty(8, 56, 6, 60, device="cuda")
    eng.randn(a, 8, 1234, 0, st)
    b = torch.empty(4, 56, 6, 60, device="cuda")
    eng.randn(b, 4, 1234, 4, st)
    assert torch.equal(a[4:], b)                       # shard [4,8) of an 8-batch == 4-batch at offset 4
    c = torch.empty_like(a)
    eng.randn(c, 8, 1235, 0, st)
    assert not torch.equal(a, c)
    n = a.numel()
    assert abs(a.mean().item()) < 4 / n ** 0.5 and abs(a.var().item() - 1) < 0.02
    assert abs((a ** 3).mean().item()) < 0.05 and abs((a ** 4).mean().item() - 3) < 0.1
    # Box-Muller on the hardware transcendentals (rgn_sampler.h): tails and the independence of the (cos, sin) pair
    flat = a.reshape(-1, 60)
    assert abs((flat[:, 0::2] * flat[:, 1::2]).mean().item()) < 5e-3                       # adjacent frames = the two outputs of one pair
    assert abs((a.abs() > 3).float().mean().item() - 2.6998e-3) < 3e-4 and a.abs().max().item() < 6.5
    assert torch.isfinite(a).all()
    # sampling with Philox: same seed -> same samples; sharded == unsharded
    y = {"cmotion": torch.from_numpy(synth.make_cmotion(cfg, 8)).cuda()}
    s1 = diffusion.p_sample_loop(model, (8, 56, 6, 60), clip_denoised=False, model_kwargs={"y": y}, seed=77)
    s2 = diffusion.p_sample_loop(model, (8, 56, 6, 60), clip_denoised=False, model_kwargs={"y": y}, seed=77)
    assert torch.equal(s1, s2)
    y2 = {"cmotion": y["cmotion"][4:].contiguous()}
    s3 = diffusion.p_sample_loop(model, (4, 56, 6, 60), clip_denoised=False, model_kwargs={"y": y2}, seed=77, sample_offset=4)
    assert torch.allclose(s1[4:], s3, atol=1e-5)
    assert torch.isfinite(s1).all()


def test_postproc_rows(golden):
    g = golden("postproc")
    from regennet_amd import synth
    cfg = synth.get_config("tiny")
    model, _ = build_hip(cfg, synth.make_state_dict(cfg, seed=0))
    eng, _ = model._get_engine(1)
    st = torch.cuda.current_stream().cuda_stream
    d6 = torch.from_numpy(g["d6"]).cuda().contiguous()
    mat = torch.empty(d6.shape[:-1] + (3, 3), device="cuda")
    eng.rot6d_to_matrix(d6, mat, d6.numel() // 6, st)
    assert np.abs(mat.cpu().numpy() - g["mats"]).max() < 1e-6
    for xk, gk in (("x", "gf"), ("x3", "gf3")):
        x = torch.from_numpy(g[xk]).cuda().contiguous()
        out = torch.empty_like(x)
        eng.gaussian_filter1d(x, out, x.numel() // x.shape[-1], x.shape[-1], 1.0, st)
        assert np.abs(out.cpu().numpy() - g[gk]).max() < 1e-6


def test_boundary_protocol_and_errors():
    """Model/diffusion object protocol of SURVEY.md §8b and error behaviour of the C-ABI."""
    from regennet_amd import _lib, synth
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from regennet_amd.utils.model_util import load_model_wo_clip
    cfg = synth.get_config("tiny")
    sd = synth.make_state_dict(cfg, seed=0)
    model, diffusion = build_hip(cfg, sd, resp="ddim5")
    assert next(model.parameters()).device.type == "cuda"
    assert (model.njoints, model.nfeats, model.data_rep, model.cond_mode) == (5, 6, "rot6d", "action")
    assert set(model.state_dict().keys()) == set(sd.keys())
    with pytest.raises(AssertionError):                       # unexpected key (model_util.py:7)
        load_model_wo_clip(model, {**{k: torch.from_numpy(v) for k, v in sd.items()}, "bogus.weight": torch.zeros(1)})
    load_model_wo_clip(model, {**{k: torch.from_numpy(v) for k, v in sd.items()}, })
    model.to("cuda:0")
    B = 2
    y = y_to_device({"cmotion": synth.make_cmotion(cfg, B), "action": synth.make_actions(cfg, B)})
    with pytest.raises(AssertionError):                       # shape mismatch
        diffusion.p_sample_loop(model, (B, 5, 6, 9), clip_denoised=False, model_kwargs={"y": y})
    with pytest.raises(NotImplementedError):
        diffusion.ddim_sample_loop(model, (B, 5, 6, 8), model_kwargs={"y": y}, dump_steps=[1])
    with pytest.raises(KeyError):                             # guided needs y['scale'] (cfg_sampler.py:31)
        diffusion.p_sample_loop(ClassifierFreeSampleModel(model), (B, 5, 6, 8), clip_denoised=False, model_kwargs={"y": y})
    dumped = diffusion.p_sample_loop(model, (B, 5, 6, 8), clip_denoised=False, model_kwargs={"y": y}, dump_steps=[0, 4], seed=3)
    assert len(dumped) == 2 and dumped[0].shape == (B, 5, 6, 8)
    clipped = diffusion.p_sample_loop(model, (B, 5, 6, 8), clip_denoised=True, model_kwargs={"y": y}, seed=3)
    assert torch.isfinite(clipped).all()
    # y is never mutated
    assert set(y.keys()) == {"cmotion", "action"}
    # raw C-ABI error codes
    eng = _lib.Engine(cfg, 2, 0, "f32")
    with pytest.raises(_lib.RgnError) as e:
        eng.load_weight("not.a.key", np.zeros((1,), np.float32))
    assert e.value.code == -2
    with pytest.raises(_lib.RgnError) as e:
        eng.load_weight("fuse_process.bias", np.zeros((3,), np.float32))
    assert e.value.code == -3
    eng.load_weight("clip_model.anything", np.zeros((3,), np.float32))   # accepted and ignored
    with pytest.raises(_lib.RgnError) as e:
        eng.finalize()
    assert e.value.code == -4 and "missing keys" in str(e.value)
    eng.close()


def test_cgenerate_cli_synthetic(tmp_path):
    """The cgenerate-style entry point end to end (synthetic checkpoint + clips, ddim5, CFG)."""
    from regennet_amd.sample import cgenerate
    out = cgenerate.main(["--synthetic", "--num_samples", "3", "--num_repetitions", "2", "--timestep_respacing", "ddim5",
                          "--use_ddim", "--guidance_param", "2.5", "--output_dir", str(tmp_path)])
    res = np.load(out, allow_pickle=True).item()
    assert res["output"].shape == (6, 56, 6, 60) and res["cmotion"].shape == (6, 56, 6, 60)
    assert np.isfinite(res["output"]).all()


def test_weight_blob_view_transfers_a_checkpoint():
    """The multi-GPU start-up path: copying rank 0's packed blob into another engine (what the RCCL broadcast does)
    makes that engine reproduce rank 0's outputs bit for bit."""
    from regennet_amd import synth
    from regennet_amd.utils import dist_util
    cfg = synth.get_config("tiny")
    ma, da = build_hip(cfg, synth.make_state_dict(cfg, seed=0), resp="ddim5", precision="bf16x3")
    mb, db = build_hip(cfg, synth.make_state_dict(cfg, seed=123), resp="ddim5", precision="bf16x3")
    B = 2
    y = y_to_device({"cmotion": synth.make_cmotion(cfg, B), "action": synth.make_actions(cfg, B)})
    kw = dict(clip_denoised=False, model_kwargs={"y": y}, seed=5)
    ea, _ = ma._get_engine(B)
    eb, _ = mb._get_engine(B)
    out_a = da.ddim_sample_loop(ma, (B, 5, 6, 8), **kw)
    out_b0 = db.ddim_sample_loop(mb, (B, 5, 6, 8), **kw)
    assert not torch.allclose(out_a, out_b0)
    (pa, na), (pb, nb) = ea.weight_blob(), eb.weight_blob()
    assert na == nb and na > 0
    va, vb = dist_util.device_view(pa, na, "cuda:0"), dist_util.device_view(pb, nb, "cuda:0")
    assert va.dtype == torch.uint8 and va.numel() == na and va.data_ptr() == pa
    vb.copy_(va)
    torch.cuda.synchronize()
    eb.set_schedule(db.timestep_map, db._engine_tables(), db._sched_token)   # per-schedule tables depend on the weights
    mb._cond_key = None                                                      # ... and so does the hoisted condition
    out_b1 = db.ddim_sample_loop(mb, (B, 5, 6, 8), **kw)
    assert torch.equal(out_a, out_b1)


def test_two_shards_after_a_blob_transfer_reproduce_the_unsharded_batch():
    """What two ranks of a multi-GPU run do, on one GPU: engine B starts from another checkpoint, receives engine A's packed
    blob (the RCCL broadcast), then A samples shard [0, B/2) and B shard [B/2, B) with the global sample offset: together
    they must equal the unsharded B-batch BIT FOR BIT (schedule tables and hoisted condition re-derived after the transfer)."""
    from regennet_amd import synth
    from regennet_amd.utils import dist_util
    cfg = synth.get_config("ntu_action", layers=2)
    ma, da = build_hip(cfg, synth.make_state_dict(cfg, seed=0), resp="50", precision="bf16_x3tail")
    mb, db = build_hip(cfg, synth.make_state_dict(cfg, seed=77), resp="50", precision="bf16_x3tail")
    B, half = 6, 3
    y = y_to_device({"cmotion": synth.make_cmotion(cfg, B, seed=8), "action": synth.make_actions(cfg, B, seed=9)})
    shape = lambda n: (n, 56, 6, 60)   # noqa: E731
    full = da.p_sample_loop(ma, shape(B), clip_denoised=False, model_kwargs={"y": y}, seed=21)
    ea, _ = ma._get_engine(B)
    eb, _ = mb._get_engine(half)
    (pa, na), (pb, nb) = ea.weight_blob(), eb.weight_blob()
    dist_util.device_view(pb, nb, "cuda:0").copy_(dist_util.device_view(pa, na, "cuda:0"))
    torch.cuda.synchronize()
    eb.schedule_id = None                                    # re-derive the schedule tables (dist_util.sync_model_weights marks engines stale instead)
    ya = {k: v[:half].contiguous() for k, v in y.items()}
    yb = {k: v[half:].contiguous() for k, v in y.items()}
    sa = da.p_sample_loop(ma, shape(half), clip_denoised=False, model_kwargs={"y": ya}, seed=21, sample_offset=0)
    sb = db.p_sample_loop(mb, shape(B - half), clip_denoised=False, model_kwargs={"y": yb}, seed=21, sample_offset=half)
    assert torch.equal(torch.cat([sa, sb]), full)


def test_chain_count_does_not_change_results(golden, monkeypatch):
    """1, 2 or 4 concurrent kernel chains (REGENNET_STREAMS) are a scheduling choice only: bit-identical samples."""
    g = golden("ntu_ddpm50")
    cfg, sd, y, tape = fixture_inputs(g, loop=True)
    outs = []
    for n in ("1", "2", "4"):
        monkeypatch.setenv("REGENNET_STREAMS", n)
        model, diffusion = build_hip(cfg, sd, resp="50", precision="bf16x3/throughput")
        outs.append(diffusion.p_sample_loop(model, (2, 56, 6, 60), clip_denoised=False, model_kwargs={"y": y_to_device(y)},
                                            noise_tape=torch.from_numpy(tape)))
        model._engine.close()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert np.abs(outs[0].cpu().numpy() - g["final"]).max() < 1e-3


def test_big_gemm_tiles_meet_the_same_bound(golden, monkeypatch):
    """Launches of >= 7000 rows per chain use the 256x256 GEMM tile; forced here on small goldens (edge tiles included)."""
    monkeypatch.setenv("REGENNET_BIG_TILE_ROWS", "1")
    for name in ("ntu_ddpm50", "ntu_action_ddim100_cfg", "text150_ddim50_cfg"):
        g = golden(name)
        cfg, sd, y, tape = fixture_inputs(g, loop=True)
        model, diffusion = build_hip(cfg, sd, resp=str(g["resp"]), precision="bf16x3/throughput")
        fm = _wrap(model, bool(g["guided"]))
        fn = diffusion.p_sample_loop if str(g["mode"]) == "ddpm" else diffusion.ddim_sample_loop
        out = fn(fm, (int(g["B"]), 56, 6, cfg["num_frames"]), clip_denoised=False, model_kwargs={"y": y_to_device(y)},
                 noise_tape=torch.from_numpy(tape))
        assert np.abs(out.cpu().numpy() - g["final"]).max() < 1e-3
        model._engine.close()


@pytest.mark.parametrize("precision,tail", [("bf16x3", None), ("bf16_x3tail", 2)])
def test_full_size_batch_is_row_independent(monkeypatch, precision, tail):
    """BASELINE configs[1] size (B=256, NTU): every sample's chain is independent, so sample b of a 256-batch must equal
    the same sample drawn alone with the same Philox key (sample_offset=b) — a size-independent property that checks
    tiling, chain splitting and row mapping at the full bench size without needing a 256-sample reference run.
    ("bf16_x3tail", 2): 3 of the 5 steps run the plain-bf16 phase kernels, 2 the split-bf16 ones. The engine picks the kernel form
    by the size of the evaluation - one workgroup per sample from 64 samples on, kernel per stage below - and the forms differ by
    bf16 roundings: REGENNET_LAYERS_MIN_B=1 gives the single-sample runs the form of the batch.)"""
    from regennet_amd import synth
    monkeypatch.setenv("REGENNET_LAYERS_MIN_B", "1")
    cfg = synth.get_config("ntu")
    sd = synth.make_state_dict(cfg, seed=0)
    model, diffusion = build_hip(cfg, sd, resp="ddim5", precision=precision + "/throughput", x3_tail=tail)   # (the B = 1 runs too)
    B = 256
    cm = torch.from_numpy(synth.make_cmotion(cfg, B, seed=1)).cuda()
    full = diffusion.ddim_sample_loop(model, (B, 56, 6, 60), clip_denoised=False, model_kwargs={"y": {"cmotion": cm}}, seed=9)
    assert torch.isfinite(full).all()
    for b in (0, 63, 64, 129, 255):          # first/last rows of different chains
        one = diffusion.ddim_sample_loop(model, (1, 56, 6, 60), clip_denoised=False,
                                         model_kwargs={"y": {"cmotion": cm[b:b + 1].contiguous()}}, seed=9, sample_offset=b)
        assert torch.allclose(full[b:b + 1], one, atol=2e-5), (b, (full[b:b + 1] - one).abs().max().item())
    # guided, ragged batch that does not divide into the chains evenly
    cfg2 = synth.get_config("ntu_action")
    model2, diffusion2 = build_hip(cfg2, synth.make_state_dict(cfg2, seed=0), resp="ddim5", precision=precision + "/throughput", x3_tail=tail)
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    g2 = ClassifierFreeSampleModel(model2)
    B2 = 37
    y2 = {"cmotion": torch.from_numpy(synth.make_cmotion(cfg2, B2, seed=3)).cuda(),
          "action": torch.from_numpy(synth.make_actions(cfg2, B2, seed=4)).cuda(), "scale": torch.full((B2,), 2.5, device="cuda")}
    full2 = diffusion2.ddim_sample_loop(g2, (B2, 56, 6, 60), clip_denoised=False, model_kwargs={"y": y2}, seed=11)
    for b in (0, 18, 36):
        yb = {k: v[b:b + 1].contiguous() for k, v in y2.items()}
        one = diffusion2.ddim_sample_loop(g2, (1, 56, 6, 60), clip_denoised=False, model_kwargs={"y": yb}, seed=11, sample_offset=b)
        assert torch.allclose(full2[b:b + 1], one, atol=2e-5), (b, (full2[b:b + 1] - one).abs().max().item())


@pytest.mark.parametrize("case", range(4))
def test_default_precision_schedule_on_random_8_layer_cases(monkeypatch, case):
    """The DEFAULT precision schedule (plain-bf16 bulk + split-bf16 tail: what every caller gets) against the oracle on random 8-layer
    models at S >= 20 - random batch, length (52 .. 64 tokens, with and without the emb_trans_dec token), guidance with per-sample scales,
    sampler, and both kernel forms of the bulk phase (one workgroup per sample forced on for these test-sized batches in the odd cases,
    kernel per stage in the even ones). The fixed goldens pin the shipped shapes; this pins the schedule away from them."""
    from oracle import regennet_oracle as orc
    from regennet_amd import synth
    rng = np.random.default_rng(4200 + case)
    T = int(rng.choice([52, 57, 60, 63, 64]))
    etd = bool(rng.integers(0, 2)) and T < 64
    B = int(rng.integers(1, 5))
    guided = bool(rng.integers(0, 2))
    sampler = str(rng.choice(["ddpm", "ddim"]))
    S = int(rng.integers(20, 27))
    cfg = synth.get_config("ntu_action", num_frames=T, emb_trans_dec=etd)
    assert cfg["layers"] == 8
    sd = synth.make_state_dict(cfg, seed=300 + case)
    resp = f"ddim{S}" if sampler == "ddim" else str(S)
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=case), "action": synth.make_actions(cfg, B, seed=case + 1)}
    if guided:
        y["scale"] = np.linspace(1.0, 2.5, B).astype(np.float32)
    tape = synth.make_noise_tape(cfg, B, S, seed=case + 2)
    ref = orc.sample_loop(sd, cfg, orc.make_schedule("cosine", resp), tape, {k: torch.from_numpy(v) for k, v in y.items()},
                          mode=sampler, guided=guided).numpy()
    monkeypatch.setenv("REGENNET_LAYERS_MIN_B", "1" if case % 2 else "100000")
    model, diffusion = build_hip(cfg, sd, resp=resp, precision="bf16_x3tail/throughput")
    model._get_engine(B)
    monkeypatch.delenv("REGENNET_LAYERS_MIN_B")
    fm = _wrap(model, guided)
    fn = diffusion.p_sample_loop if sampler == "ddpm" else diffusion.ddim_sample_loop
    out = fn(fm, (B, 56, 6, T), clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
    err = float(np.abs(out.cpu().numpy() - ref).max())
    print(f"\n[default schedule, random 8-layer case {case}] T={T} etd={int(etd)} B={B} guided={int(guided)} {sampler} S={S} "
          f"{'k_layers' if case % 2 else 'kernel per stage'}: {err:.2e}")
    assert err < 1e-3, err
    model._engine.close()


@pytest.mark.parametrize("name", ["ntu_eval_ddim5", "ntu_eval_5", "ntu_action_eval_ddim5"])
def test_reference_evaluation_setting_switch_point_sweep(golden, monkeypatch, name):
    """The reference's shipped evaluation setting (README.md:134-137, eval/a2m/stgcn_eval.py:61,69): `--timestep_respacing ddim5`
    (and the plain 5-step spacing) through p_sample_loop, 8-layer NTU model, against the reference's own outputs - for every
    precision-schedule switch point 0 .. 5, on the throughput kernels and with the one-kernel decoder stack forced on (a
    test-sized batch). The default (3 split-bf16 steps for schedules of up to 10) and every longer tail must stay at the level
    of the all-split run (< 1.5e-4, bound 1e-3); what fewer split-bf16 steps cost is printed."""
    g = golden(name)
    cfg, sd, y, tape = fixture_inputs(g, loop=True)
    S = int(g["S"])
    assert S == 5 and default_tail(S) == 3
    shape = (int(g["B"]), cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    errs = {}
    for layers_on in (False, True):
        for tail in (0, 1, 2, None, 5):                       # (None = the default = 3)
            monkeypatch.setenv("REGENNET_LAYERS_MIN_B", "1" if layers_on else "100000")
            model, diffusion = build_hip(cfg, sd, resp=str(g["resp"]), precision="bf16_x3tail/throughput", x3_tail=tail)
            model._get_engine(shape[0])
            monkeypatch.delenv("REGENNET_LAYERS_MIN_B")
            out = diffusion.p_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
            errs[(layers_on, tail)] = float(np.abs(out.cpu().numpy() - g["final"]).max())
            model._engine.close()
    for layers_on in (False, True):
        print(f"\n[5-step evaluation schedule] {name} {'k_layers' if layers_on else 'kernel per stage'}: " +
              ", ".join(f"tail {t}: {errs[(layers_on, t)]:.2e}" for t in (0, 1, 2, None, 5)))
        for t in (None, 5):
            assert errs[(layers_on, t)] < 1.5e-4, (layers_on, t, errs[(layers_on, t)])
        assert errs[(layers_on, 2)] < 3.5e-4


@pytest.mark.parametrize("sampler,clip,guided", [("ddpm", False, False), ("ddim", True, False), ("ddim", False, True), ("ddpm", True, True)])
def test_fused_step_boundary_matches_the_three_kernel_form(monkeypatch, sampler, clip, guided):
    """k_step (plain-bf16 phase, throughput kernels: output projection + sampler update + next input embedding in one kernel;
    with guidance both evaluations' output projections and the combination x0_u + scale (x0_c - x0_u)) against the same loop
    with the three separate launches (REGENNET_NO_STEP_FUSION=1), on-device Philox noise: same noise stream, same sampler
    arithmetic, so the results differ only by the plain-bf16 phase's rounding (the fused kernel rounds h' to bf16 twice) and
    end within the parity margin of each other after the split-bf16 tail. And the quad-shared Philox draw of k_step is
    bit-identical to the per-element one (REGENNET_STEP_NO_QUADS=1)."""
    from regennet_amd import synth
    cfg = synth.get_config("ntu_action" if guided else "ntu")
    sd = synth.make_state_dict(cfg, seed=0)
    B = 5                                       # 300 rows: 4 full tiles + a partial one, tiles straddling samples
    y = {"cmotion": torch.from_numpy(synth.make_cmotion(cfg, B, seed=1)).cuda()}
    if guided:
        y["action"] = torch.from_numpy(synth.make_actions(cfg, B, seed=2)).cuda()
        y["scale"] = torch.linspace(1.5, 3.5, B).cuda()          # per-sample scales
    outs = {}
    for tag, env in (("fused", None), ("per_element_noise", "REGENNET_STEP_NO_QUADS"), ("three_kernels", "REGENNET_NO_STEP_FUSION")):
        if env:
            monkeypatch.setenv(env, "1")
        model, diffusion = build_hip(cfg, sd, resp="50" if sampler == "ddpm" else "ddim50", precision="bf16_x3tail/throughput")
        model._get_engine(B)                    # (the switches are read when the engine is built)
        if env:
            monkeypatch.delenv(env)
        fm = _wrap(model, guided)
        fn = diffusion.p_sample_loop if sampler == "ddpm" else diffusion.ddim_sample_loop
        outs[tag] = fn(fm, (B, 56, 6, 60), clip_denoised=clip, model_kwargs={"y": y}, seed=3)
        model._engine.close()
    assert torch.isfinite(outs["fused"]).all()
    assert torch.equal(outs["fused"], outs["per_element_noise"])
    dev = (outs["fused"] - outs["three_kernels"]).abs().max().item()
    print(f"\n[fused step boundary] {sampler} clip={clip} guided={guided} vs three kernels: {dev:.2e}")
    assert 0.0 < dev < 5e-4


def test_engine_selection_can_change_between_calls(golden):
    """rgn_set_small_batch_rows on a live engine: captured graphs belong to the engine they were recorded with, so switching
    drops them. Small-batch -> throughput -> small-batch on one model: the first and third results are bit-identical, the
    second agrees within the mode's error, all three meet the reference bound."""
    g = golden("ntu_ddpm50")
    cfg, sd, y, tape = fixture_inputs(g, loop=True)
    model, diffusion = build_hip(cfg, sd, resp="50", precision="bf16_x3tail")
    kw = dict(clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
    outs = []
    for rows in (None, 0, None):
        model.small_batch_rows = rows
        outs.append(diffusion.p_sample_loop(model, (2, 56, 6, 60), **kw))
    assert torch.equal(outs[0], outs[2])
    assert not torch.equal(outs[0], outs[1]) and (outs[0] - outs[1]).abs().max().item() < 5e-4
    for o in outs:
        assert np.abs(o.cpu().numpy() - g["final"]).max() < 1e-3


@pytest.mark.parametrize("config,B,T", [("ntu_action", 5, 60), ("chi3d", 2, 150)])
def test_small_batch_engine_is_bit_exact_under_batch_composition(config, B, T):
    """The small-batch kernels (rgn_sb.hip) accumulate every output element in a fixed order that does not depend on which
    rows share its tile, so sample b of a batch equals the same sample drawn alone BIT FOR BIT — guided (2B rows: up to
    600 of the 640 the engine takes; 32- and 64-row tiles) and unguided, across both phases of the precision schedule."""
    from regennet_amd import synth
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    cfg = synth.get_config(config)
    model, diffusion = build_hip(cfg, synth.make_state_dict(cfg, seed=0), resp="ddim5", precision="bf16_x3tail", x3_tail=2)
    y = {"cmotion": torch.from_numpy(synth.make_cmotion(cfg, B, seed=1)).cuda(),
         "action": torch.from_numpy(synth.make_actions(cfg, B, seed=2)).cuda(), "scale": torch.full((B,), 2.5, device="cuda")}
    for fm in (model, ClassifierFreeSampleModel(model)):
        full = diffusion.ddim_sample_loop(fm, (B, 56, 6, T), clip_denoised=False, model_kwargs={"y": y}, seed=13)
        assert torch.isfinite(full).all()
        for b in (0, 1, B - 1):
            yb = {k: v[b:b + 1].contiguous() for k, v in y.items()}
            one = diffusion.ddim_sample_loop(fm, (1, 56, 6, T), clip_denoised=False, model_kwargs={"y": yb}, seed=13, sample_offset=b)
            assert torch.equal(full[b:b + 1], one), (b, (full[b:b + 1] - one).abs().max().item())


@pytest.mark.parametrize("precision,tail", [("bf16x3", None), ("bf16_x3tail", 2)])
def test_chi3d_full_size_shard_is_row_independent(precision, tail):
    """BASELINE configs[3] per-GPU shard (Chi3D T=150, B=128 = 1024 / 8): the long-sequence kernels (in_proj GEMM with the
    attention-ready scatter + k_attn_x3) at full size, guided and unguided, via the same row-independence property."""
    from regennet_amd import synth
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    cfg = synth.get_config("chi3d")
    model, diffusion = build_hip(cfg, synth.make_state_dict(cfg, seed=0), resp="ddim5", precision=precision + "/throughput", x3_tail=tail)
    B = 128
    y = {"cmotion": torch.from_numpy(synth.make_cmotion(cfg, B, seed=1)).cuda(),
         "action": torch.from_numpy(synth.make_actions(cfg, B, seed=2)).cuda(), "scale": torch.full((B,), 2.5, device="cuda")}
    for fm in (model, ClassifierFreeSampleModel(model)):
        full = diffusion.ddim_sample_loop(fm, (B, 56, 6, 150), clip_denoised=False, model_kwargs={"y": y}, seed=13)
        assert torch.isfinite(full).all()
        for b in (0, 31, 32, 127):
            yb = {k: v[b:b + 1].contiguous() for k, v in y.items()}
            one = diffusion.ddim_sample_loop(fm, (1, 56, 6, 150), clip_denoised=False, model_kwargs={"y": yb}, seed=13, sample_offset=b)
            assert torch.allclose(full[b:b + 1], one, atol=2e-5), (b, (full[b:b + 1] - one).abs().max().item())


_BENCH_SHAPE_REF = {}


def _bench_shape_reference(cfg_name, mode, resp, guided, B):
    """Inputs + oracle result of one bench-shape case, computed once per session (the four precision cases share them: the oracle's
    B=256 run is ~20 s of host CPU)."""
    key = (cfg_name, mode, resp, guided, B)
    if key not in _BENCH_SHAPE_REF:
        from oracle import regennet_oracle as orc
        from regennet_amd import synth
        cfg = synth.get_config(cfg_name)
        sd = synth.make_state_dict(cfg, seed=0)
        y = {"cmotion": synth.make_cmotion(cfg, B, seed=41)}
        if guided:
            y["action"] = synth.make_actions(cfg, B, seed=42)
            y["scale"] = np.full((B,), 2.5, dtype=np.float32)
        tape = synth.make_noise_tape(cfg, B, 3, seed=43)
        ref = orc.sample_loop(sd, cfg, orc.make_schedule("cosine", resp), tape, {k: torch.from_numpy(v) for k, v in y.items()},
                              mode=mode, guided=guided).numpy()
        _BENCH_SHAPE_REF[key] = (cfg, sd, y, tape, ref)
    return _BENCH_SHAPE_REF[key]


@pytest.mark.parametrize("precision,tail,tol", [("f32", None, 2e-4), ("bf16x3", None, 1e-3), ("bf16_x3tail", None, 1e-3),
                                                 ("bf16_x3tail", 0, 0.15)])
def test_bench_shape_against_the_oracle(precision, tail, tol):
    """HIP vs oracle AT THE BENCH SHAPE (B=256, NTU): 3 DDPM steps unguided (4 kernel chains + the step graph) and 3 DDIM
    steps guided (512 rows per evaluation -> the 256x256 GEMM tile). The last case runs all three steps in the plain-bf16
    phase of the precision schedule; three steps cannot contract its rounding, so it only has to stay at bf16 level."""
    from oracle import regennet_oracle as orc
    from regennet_amd import synth
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    B = 256
    for cfg_name, mode, resp, guided in (("ntu", "ddpm", "3", False), ("ntu_action", "ddim", "ddim3", True)):
        cfg, sd, y, tape, ref = _bench_shape_reference(cfg_name, mode, resp, guided, B)
        model, diffusion = build_hip(cfg, sd, resp=resp, precision=precision, x3_tail=tail)
        fm = ClassifierFreeSampleModel(model) if guided else model
        fn = diffusion.p_sample_loop if mode == "ddpm" else diffusion.ddim_sample_loop
        out = fn(fm, (B, 56, 6, 60), clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
        err = float(np.abs(out.cpu().numpy() - ref).max())
        print(f"\n[bench shape vs oracle] {cfg_name} {mode} guided={guided} {precision} tail={tail}: {err:.2e}")
        assert err < tol, (cfg_name, precision, tail, err)
        model._engine.close()


def test_bench_shape_bulk_phase_against_the_oracle():
    """The plain-bf16 bulk-phase kernels (k_mlp, k_qkv_attn_rs, k_step: 99 % of the timed region of bench.py) AT THE BENCH SHAPE
    inside the 1e-3 bound: 16-step schedules at B=256 under the DEFAULT precision schedule = 11 plain-bf16 + 5 split-bf16
    steps, unguided DDPM (k_step) and guided DDIM (k_step<., true>), against the oracle on identical noise."""
    from oracle import regennet_oracle as orc
    from regennet_amd import synth
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    B = 256
    assert default_tail(16) == 5
    for cfg_name, mode, resp, guided in (("ntu", "ddpm", "16", False), ("ntu_action", "ddim", "ddim16", True)):
        cfg = synth.get_config(cfg_name)
        sd = synth.make_state_dict(cfg, seed=0)
        y = {"cmotion": synth.make_cmotion(cfg, B, seed=51)}
        if guided:
            y["action"] = synth.make_actions(cfg, B, seed=52)
            y["scale"] = np.full((B,), 2.5, dtype=np.float32)
        tape = synth.make_noise_tape(cfg, B, 16, seed=53)
        # the oracle (host CPU) runs every 8th motion - motions are independent, 32 of them sit on 32 different workgroups of all 8 XCDs
        # (every 4th until round 6: the oracle's seconds are most of this suite's wall time) - the HIP path runs the full bench batch
        idx = np.arange(0, B, 8)
        ref = orc.sample_loop(sd, cfg, orc.make_schedule("cosine", resp), np.ascontiguousarray(tape[:, idx]),
                              {k: torch.from_numpy(np.ascontiguousarray(v[idx])) for k, v in y.items()}, mode=mode, guided=guided).numpy()
        model, diffusion = build_hip(cfg, sd, resp=resp, precision="bf16_x3tail")
        fm = ClassifierFreeSampleModel(model) if guided else model
        fn = diffusion.p_sample_loop if mode == "ddpm" else diffusion.ddim_sample_loop
        out = fn(fm, (B, 56, 6, 60), clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
        assert torch.isfinite(out).all()
        err = float(np.abs(out.cpu().numpy()[idx] - ref).max())
        print(f"\n[bench shape, 11 bulk + 5 tail steps vs oracle] {cfg_name} {mode} guided={guided}: {err:.2e}")
        assert err < 1e-3, (cfg_name, err)
        model._engine.close()


@pytest.mark.parametrize("cfg_name,B,guided,frames", [("ntu", 16, False, None), ("ntu", 3, False, None), ("ntu_action", 5, True, None),
                                                      ("chi3d", 3, False, None), ("ntu", 7, False, 40)])
def test_split_bf16_layer_tail_kernel_matches_the_five_kernel_form(cfg_name, B, guided, frames, monkeypatch):
    """k_mlp_x3 (rgn_mlp_x3.hip: the split-bf16 layer tail as ONE row-persistent kernel, 32-row tiles) against the kernels it replaced
    (k_gemm_x3 x 3 + k_layernorm x 2 per layer, REGENNET_MLP_X3=0) and against the oracle: uniform split-bf16 arithmetic, throughput engine,
    row counts that end in a partial tile (B = 3: 180 rows; chi3d: 450) and tiles that straddle two motions (T = 40 / 60 / 150 against 32-row tiles),
    per-sample condition vectors, guidance."""
    from oracle import regennet_oracle as orc
    from regennet_amd import synth
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    cfg = synth.get_config(cfg_name)
    sd = synth.make_state_dict(cfg, seed=7)
    if frames:                                                   # a shorter motion than the checkpoint's (--motion_length): 40-row motions against 32-row tiles
        cfg = dict(cfg, num_frames=frames)
    T = cfg["num_frames"]
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=61)}
    if cfg["cond_mode"] == "action":
        y["action"] = synth.make_actions(cfg, B, seed=62)
    if guided:
        y["scale"] = np.linspace(1.0, 3.0, B).astype(np.float32)
    resp, mode = ("ddim3", "ddim") if guided else ("3", "ddpm")
    tape = synth.make_noise_tape(cfg, B, 3, seed=63)
    ref = orc.sample_loop(sd, cfg, orc.make_schedule("cosine", resp), tape, {k: torch.from_numpy(v) for k, v in y.items()},
                          mode=mode, guided=guided).numpy()
    outs = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("REGENNET_MLP_X3", flag)               # read when the engine is built
        model, diffusion = build_hip(cfg, sd, resp=resp, precision="bf16x3/throughput")
        fm = ClassifierFreeSampleModel(model) if guided else model
        fn = diffusion.p_sample_loop if mode == "ddpm" else diffusion.ddim_sample_loop
        outs[flag] = fn(fm, (B, cfg["njoints"], cfg["nfeats"], T), clip_denoised=False, model_kwargs={"y": y_to_device(y)},
                        noise_tape=torch.from_numpy(tape)).cpu().numpy()
        model._engine.close()
    e1, e0, d = np.abs(outs["1"] - ref).max(), np.abs(outs["0"] - ref).max(), np.abs(outs["1"] - outs["0"]).max()
    print(f"\n[k_mlp_x3] {cfg_name} B={B} guided={guided}: vs oracle {e1:.2e} (five-kernel form {e0:.2e}), the two forms differ by {d:.2e}")
    assert e1 < 1e-3 and e0 < 1e-3 and d < 2e-4 and e1 < 2.0 * e0 + 2e-5


@pytest.mark.parametrize("cfg_name,B,guided,frames,precision", [("ntu", 16, False, None, "bf16x3/throughput"), ("ntu", 3, False, None, "bf16x3/throughput"),
                                                                ("ntu_action", 5, True, None, "bf16x3/throughput"), ("ntu", 7, False, 40, "bf16x3/throughput"),
                                                                ("ntu", 300, False, None, "bf16_x3tail/throughput"), ("ntu_action", 140, True, None, "bf16_x3tail/throughput")])
def test_split_bf16_qkv_attention_register_streamed_form_equals_the_dma_form(cfg_name, B, guided, frames, precision):
    """k_qkv_attn_rs_x3 (round 6: the split phase's in_proj + attention with the hi and lo weight fragment planes streamed into register rings, one sample per
    four-wave workgroup) against k_qkv_attn<true> (direct-to-LDS operands, two samples per workgroup; engine option QKV_X3_DMA = 1): every accumulator sees
    the same MFMAs in the same order, so the two forms agree BIT FOR BIT - odd batches (the DMA form pads its last pair), 40-frame motions, guidance, one and
    two heads per workgroup (B < / >= 256 evaluations), the uniform split mode and the tail of the default schedule - and against the oracle."""
    from oracle import regennet_oracle as orc
    from regennet_amd import synth
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    cfg = synth.get_config(cfg_name)
    sd = synth.make_state_dict(cfg, seed=9)
    if frames:
        cfg = dict(cfg, num_frames=frames)
    T = cfg["num_frames"]
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=71)}
    if cfg["cond_mode"] == "action":
        y["action"] = synth.make_actions(cfg, B, seed=72)
    if guided:
        y["scale"] = np.linspace(1.0, 3.0, B).astype(np.float32)
    resp, mode = ("ddim3", "ddim") if guided else ("3", "ddpm")
    tape = synth.make_noise_tape(cfg, B, 3, seed=73)
    outs, names = {}, {}
    for dma in (0, 1):
        model, diffusion = build_hip(cfg, sd, resp=resp, precision=precision, x3_tail=2 if "tail" in precision else None, f16_steps=0 if "tail" in precision else None,
                                     engine_options={"QKV_X3_DMA": dma, "LAYERS": 0})
        fm = ClassifierFreeSampleModel(model) if guided else model
        fn = diffusion.p_sample_loop if mode == "ddpm" else diffusion.ddim_sample_loop
        outs[dma] = fn(fm, (B, cfg["njoints"], cfg["nfeats"], T), clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape)).cpu().numpy()
        model._engine.close()
    assert np.array_equal(outs[0], outs[1]), float(np.abs(outs[0] - outs[1]).max())
    if B <= 16:
        ref = orc.sample_loop(sd, cfg, orc.make_schedule("cosine", resp), tape, {k: torch.from_numpy(v) for k, v in y.items()}, mode=mode, guided=guided).numpy()
        err = float(np.abs(outs[0] - ref).max())
        print(f"\n[k_qkv_attn_rs_x3] {cfg_name} B={B} guided={guided}: vs oracle {err:.2e}, the two forms are bit-equal")
        assert err < 1e-3


def test_text150_full_size_shard_is_row_independent():
    """BASELINE configs[4] per-GPU shard at FULL size (text-conditioned, T=150, B=256 = 2048 / 8, CFG: 76 800 token rows, 1200 row
    tiles, four kernel chains, the guided fused step at 150 frames): rows of the batch against the same motion drawn alone
    with its global sample index (same Philox key), across both phases of the precision schedule."""
    from regennet_amd import synth
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    cfg = synth.get_config("text150")
    model, diffusion = build_hip(cfg, synth.make_state_dict(cfg, seed=0), resp="ddim5", precision="bf16_x3tail/throughput", x3_tail=2)
    B = 256
    y = {"cmotion": torch.from_numpy(synth.make_cmotion(cfg, B, seed=1)).cuda(),
         "text_features": torch.from_numpy(synth.make_text_features(cfg, B, seed=3)).cuda(), "scale": torch.full((B,), 2.5, device="cuda")}
    fm = ClassifierFreeSampleModel(model)
    full = diffusion.ddim_sample_loop(fm, (B, 56, 6, 150), clip_denoised=False, model_kwargs={"y": y}, seed=13)
    assert torch.isfinite(full).all()
    for b in (0, 127, 128, 255):
        yb = {k: v[b:b + 1].contiguous() for k, v in y.items()}
        one = diffusion.ddim_sample_loop(fm, (1, 56, 6, 150), clip_denoised=False, model_kwargs={"y": yb}, seed=13, sample_offset=b)
        assert torch.allclose(full[b:b + 1], one, atol=2e-5), (b, (full[b:b + 1] - one).abs().max().item())


def _redraw_tape(eng, shape, seed, S, idx):
    """x_T and the S per-step draws of the fused loop's own Philox stream (rgn_randn_step), motions `idx`: the oracle's noise tape."""
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.empty(shape, device="cuda")
    tape = np.empty((S + 1, len(idx)) + tuple(shape[1:]), dtype=np.float32)
    for k, loop_index in enumerate([-1] + list(range(S - 1, -1, -1))):     # draw order: x_T, then loop indices S-1 .. 0
        eng.randn_step(buf, shape[0], seed, 0, loop_index, st)
        tape[k] = buf[idx].cpu().numpy()
    return tape


def test_chi3d_full_size_shard_against_the_oracle_on_a_100_step_schedule():
    """BASELINE configs[3]'s per-GPU shard at its real size - Chi3D, 150 frames, B = 128: 300 row tiles in four kernel chains of k_qkv_attn_long +
    k_mlp2 + k_step per step - on a 100-step DDPM schedule (95 plain-bf16 + 5 split-bf16 steps), default engine, on-device Philox; motions 0, 24, 48, ... 120 and the
    last (every chain, both ends of the batch) against the ORACLE on the very noise the kernels drew (re-drawn through rgn_randn_step). Bound: north_star's 1e-3.
    Reference: utils/model_util.py:61-64 (num_frames = 150), diffusion/gaussian_diffusion.py:610-742."""
    from oracle import regennet_oracle as orc
    from regennet_amd import synth
    cfg = synth.get_config("chi3d")
    sd = synth.make_state_dict(cfg, seed=0)
    B, S, seed = 128, 100, 79
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=71), "action": synth.make_actions(cfg, B, seed=72)}
    model, diffusion = synth.build_model(cfg, sd, resp=str(S), precision="bf16_x3tail", device="cuda:0")
    shape = (B, 56, 6, 150)
    out = diffusion.p_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": y_to_device(y)}, seed=seed, sample_offset=0)
    assert torch.isfinite(out).all()
    plan = model._engine.plan_query(B)
    assert plan["qkv_attn"]["kernel"] == "k_qkv_attn_long" and plan["mlp"]["kernel"] == "k_mlp2" and "step_fused" in plan, plan
    idx = np.r_[np.arange(0, B, 24), B - 1]
    tape = _redraw_tape(model._engine, shape, seed, S, idx)
    ref = orc.sample_loop(sd, cfg, orc.make_schedule("cosine", str(S)), tape,
                          {k: torch.from_numpy(np.ascontiguousarray(v[idx])) for k, v in y.items()}, mode="ddpm").numpy()
    err = float(np.abs(out.cpu().numpy()[idx] - ref).max())
    print(f"\n[cfg4 shard: chi3d B = 128, 150 frames, 95 + 5 steps, on-device Philox] a subset of the motions vs oracle: {err:.2e}")
    assert err < 1e-3, err
    model._engine.close()


def test_text150_full_size_shard_against_the_oracle_on_its_own_schedule():
    """BASELINE configs[4]'s per-GPU shard EXACTLY: text-conditioned, 150 frames, B = 256, `ddim50` + guidance 2.5 (512 evaluations per step: 1200
    row tiles; 45 plain-bf16 steps through k_qkv_attn_long + k_mlp2 + the guided k_step, 5 split-bf16 steps), default engine, on-device Philox;
    every 32nd motion and the last against the ORACLE (cfg_forward, model/cfg_sampler.py:24-31) on the noise the kernels drew. Bound: 1e-3."""
    from oracle import regennet_oracle as orc
    from regennet_amd import synth
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    cfg = synth.get_config("text150")
    sd = synth.make_state_dict(cfg, seed=0)
    B, S, seed = 256, 50, 83
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=71), "text_features": synth.make_text_features(cfg, B, seed=73), "scale": np.full((B,), 2.5, np.float32)}
    model, diffusion = synth.build_model(cfg, sd, resp="ddim50", precision="bf16_x3tail", device="cuda:0")
    shape = (B, 56, 6, 150)
    out = diffusion.ddim_sample_loop(ClassifierFreeSampleModel(model), shape, clip_denoised=False, model_kwargs={"y": y_to_device(y)}, seed=seed, sample_offset=0)
    assert torch.isfinite(out).all() and diffusion.num_timesteps == S
    plan = model._engine.plan_query(B, guided=True)
    assert plan["qkv_attn"]["kernel"] == "k_qkv_attn_long" and plan["step_fused"]["kernel"] == "k_step<guided>", plan
    idx = np.r_[np.arange(0, B, 32), B - 1]
    tape = _redraw_tape(model._engine, shape, seed, S, idx)
    ref = orc.sample_loop(sd, cfg, orc.make_schedule("cosine", "ddim50"), tape,
                          {k: torch.from_numpy(np.ascontiguousarray(v[idx])) for k, v in y.items()}, mode="ddim", guided=True).numpy()
    err = float(np.abs(out.cpu().numpy()[idx] - ref).max())
    print(f"\n[cfg5 shard: text150 B = 256 + CFG, ddim50, on-device Philox] every 32nd motion + the last vs oracle: {err:.2e}")
    assert err < 1e-3, err
    model._engine.close()


def test_chi3d_1000_step_launch_sequence_rows_equal_single_motion_runs():
    """BASELINE configs[3]'s per-GPU call EXACTLY as bench.py issues it: Chi3D B = 128, the full 1000-step DDPM loop (99 ten-step graphs + 5 single
    steps of the plain-bf16 phase in four chains, then the split-bf16 tail), on-device Philox. Rows {0, 31, 32, 127} against B = 1 runs of the same
    kernels (throughput engine) with the motion's global Philox key - what bench.py's row check does on builder-run lines, inside the suite."""
    from regennet_amd import synth
    cfg = synth.get_config("chi3d")
    sd = synth.make_state_dict(cfg, seed=0)
    B = 128
    y = {"cmotion": torch.from_numpy(synth.make_cmotion(cfg, B, seed=1)).cuda(), "action": torch.from_numpy(synth.make_actions(cfg, B, seed=2)).cuda()}
    model, diffusion = synth.build_model(cfg, sd, resp="", precision="bf16_x3tail", device="cuda:0")
    full = diffusion.p_sample_loop(model, (B, 56, 6, 150), clip_denoised=False, model_kwargs={"y": y}, seed=100, sample_offset=0)
    assert torch.isfinite(full).all() and diffusion.num_timesteps == 1000
    model._engine.close()
    model1, diffusion1 = build_hip(cfg, sd, resp="", precision="bf16_x3tail/throughput")
    worst = 0.0
    for b in (0, 31, 32, 127):
        yb = {k: v[b:b + 1].contiguous() for k, v in y.items()}
        one = diffusion1.p_sample_loop(model1, (1, 56, 6, 150), clip_denoised=False, model_kwargs={"y": yb}, seed=100, sample_offset=b)
        worst = max(worst, (full[b:b + 1] - one).abs().max().item())
    print(f"\n[cfg4 launch sequence, B = 128 x 1000 steps] rows (0, 31, 32, 127) vs single-motion runs: max |dev| = {worst:.1e}")
    assert worst <= 2e-5, worst
    model1._engine.close()


@pytest.mark.parametrize("case", range(20))
def test_fuzz_parity_case(case):
    """20 seeded cases of the randomised sweep (tests/fuzz_cases.py; `tools/fuzz_parity.py` runs any number): odd batch sizes,
    8-160 frames, ff width, per-sample guidance scales, both samplers and engines, emb_trans_dec."""
    from tests.fuzz_cases import run_case
    ok, desc, _, _ = run_case(case, np.random.default_rng(1000 + case))
    print("\n" + desc)
    assert ok, desc


def test_factory_path_measures_the_switch_point_of_an_unvalidated_checkpoint(capfd):
    """A model built by the plain factory path — create_model_and_diffusion + load_model_wo_clip (utils/model_util.py:5-17), no
    precision keyword anywhere — does not trust the depth-scaled default tail on weights nobody validated: it measures the
    switch point at the first sampling call, says so once, and ends inside 1e-3 on a shallow guided model, the kind the schedule is
    most sensitive to (2 layers, ddim100 + CFG: 1.4e-3 with 5 split-bf16 steps, 8.3e-4 with 8)."""
    import types
    from oracle import regennet_oracle as orc
    from regennet_amd import synth
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from regennet_amd.utils.model_util import create_model_and_diffusion, load_model_wo_clip
    cfg = synth.get_config("ntu_action", layers=2)
    sd = synth.make_state_dict(cfg, seed=5)
    args = types.SimpleNamespace(setting="cmdm", unconstrained=False, dataset="ntu", pose_rep="rot6d", body_model="smplx", latent_dim=512,
                                 layers=2, cond_mask_prob=0.1, arch="online", cm_mode="concat", wo_pos_emb=False, emb_trans_dec=False,
                                 timestep_respacing="ddim100", noise_schedule="cosine", sigma_small=True, num_person=2)
    data = types.SimpleNamespace(dataset=types.SimpleNamespace(num_actions=cfg["num_actions"], num_person=2))
    model, diffusion = create_model_and_diffusion(args, data)
    load_model_wo_clip(model, {k: torch.from_numpy(v) for k, v in sd.items()})
    assert model.x3_tail == "auto" and model.precision == "bf16_x3tail"
    model.to("cuda:0")
    model.eval()
    B = 2
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=61), "action": synth.make_actions(cfg, B, seed=62), "scale": np.full((B,), 2.5, np.float32)}
    tape = synth.make_noise_tape(cfg, B, 100, seed=63)
    ref = orc.sample_loop(sd, cfg, orc.make_schedule("cosine", "ddim100"), tape, {k: torch.from_numpy(v) for k, v in y.items()},
                          mode="ddim", guided=True).numpy()
    out = diffusion.ddim_sample_loop(ClassifierFreeSampleModel(model), (B, 56, 6, 60), clip_denoised=False, model_kwargs={"y": y_to_device(y)},
                                     noise_tape=torch.from_numpy(tape))
    err = float(np.abs(out.cpu().numpy() - ref).max())
    log = capfd.readouterr().err
    print(f"\n[factory path] calibrated tail {model._auto_tail} of 100, error vs oracle {err:.2e}")
    assert "precision schedule calibrated" in log and model._auto_tail >= 32 and err < 1e-3, (model._auto_tail, err, log)


def test_const_noise_broadcasts_motion_0s_draw():
    """p_sample's const_noise (gaussian_diffusion.py:544-547): every motion receives motion 0's per-step draw. Tape path: equal to
    an ordinary run on a tape whose entries k >= 1 repeat motion 0's; Philox path: motions with identical condition and x_T stay
    identical through the loop (and do not without the flag). Both phases of the precision schedule, fused step included."""
    from regennet_amd import synth
    for cfg_name, prec in (("tiny", "bf16x3"), ("ntu", "bf16_x3tail/throughput")):
        cfg = synth.get_config(cfg_name)
        sd = synth.make_state_dict(cfg, seed=0)
        model, diffusion = build_hip(cfg, sd, resp="10", precision=prec, x3_tail=3 if "tail" in prec else None)
        B = 3
        shape = (B, cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
        y = {"cmotion": synth.make_cmotion(cfg, B, seed=1)}
        if cfg["cond_mode"] == "action":
            y["action"] = synth.make_actions(cfg, B, seed=2)
        tape = synth.make_noise_tape(cfg, B, 10, seed=10)
        bc = tape.copy()
        bc[1:] = tape[1:, :1]
        a = diffusion.p_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape), const_noise=True)
        b = diffusion.p_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(bc))
        assert torch.equal(a, b)
        c = diffusion.p_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape))
        assert not torch.equal(a, c)                          # the flag does not stick to the engine
        same = {k: np.repeat(v[:1], B, axis=0) for k, v in y.items()}
        x_T = torch.from_numpy(np.repeat(tape[0][:1], B, axis=0))
        d = diffusion.p_sample_loop(model, shape, noise=x_T, clip_denoised=False, model_kwargs={"y": y_to_device(same)}, seed=5, const_noise=True)
        assert torch.allclose(d[0], d[1], atol=1e-5) and torch.allclose(d[0], d[2], atol=1e-5)
        e = diffusion.p_sample_loop(model, shape, noise=x_T, clip_denoised=False, model_kwargs={"y": y_to_device(same)}, seed=5)
        assert (e[0] - e[1]).abs().max() > 1e-3
        assert torch.allclose(d[0], e[0], atol=1e-5)          # motion 0 itself is unchanged by the flag


def test_randomize_class_fails_like_the_reference_and_progressive_yields_fresh_tensors():
    """randomize_class (gaussian_diffusion.py:726-729) draws class ids for a TENSOR-valued model_kwargs['y'] from model.num_classes:
    with CMDM's dict-valued y the reference raises AttributeError at that statement; so does the mirror. The progressive
    generators yield a fresh dict of fresh tensors per step (:731-742)."""
    from regennet_amd import synth
    cfg = synth.get_config("tiny")
    model, diffusion = build_hip(cfg, synth.make_state_dict(cfg, seed=0), resp="5", precision="bf16_x3tail")
    y = y_to_device({"cmotion": synth.make_cmotion(cfg, 2), "action": synth.make_actions(cfg, 2)})
    with pytest.raises(AttributeError):
        diffusion.p_sample_loop(model, (2, 5, 6, 8), clip_denoised=False, model_kwargs={"y": y}, randomize_class=True)
    outs = list(diffusion.p_sample_loop_progressive(model, (2, 5, 6, 8), clip_denoised=False, model_kwargs={"y": y}, seed=3))
    assert len(outs) == 5 and len({o["sample"].data_ptr() for o in outs}) == 5 and len({o["pred_xstart"].data_ptr() for o in outs}) == 5
    assert not torch.equal(outs[0]["sample"], outs[-1]["sample"])
    final = diffusion.p_sample_loop(model, (2, 5, 6, 8), clip_denoised=False, model_kwargs={"y": y}, seed=3)
    assert torch.allclose(outs[-1]["sample"], final, atol=1e-3)


def test_condition_is_rebound_for_every_sampling_call():
    """Two different CPU `cmotion` / `action` tensors passed back to back (a per-batch `y` as in eval/a2m/stgcn_eval.py:41-69):
    each call must sample with ITS condition, whatever addresses the allocator hands out."""
    from regennet_amd import synth
    cfg = synth.get_config("tiny")
    sd = synth.make_state_dict(cfg, seed=0)
    model, diffusion = build_hip(cfg, sd, resp="ddim5", precision="bf16x3")
    B = 2

    def y_cpu(seed):   # function-scoped tensors: freed on return of the sampling call, their storage is reused at once
        return {"cmotion": torch.from_numpy(synth.make_cmotion(cfg, B, seed=seed)), "action": torch.full((B, 1), seed % 3)}

    outs = {}
    for seed in (5, 6, 5, 7, 6):
        out = diffusion.ddim_sample_loop(model, (B, 5, 6, 8), clip_denoised=False, model_kwargs={"y": y_cpu(seed)}, seed=1)
        if seed in outs:
            assert torch.equal(out, outs[seed]), seed
        outs[seed] = out
    assert not torch.equal(outs[5], outs[6]) and not torch.equal(outs[6], outs[7])
    # the per-step API caches the bind for an unchanged y and notices in-place edits (version counter)
    yd = y_to_device({"cmotion": synth.make_cmotion(cfg, B, seed=5), "action": synth.make_actions(cfg, B, seed=2)})
    x = torch.randn(B, 5, 6, 8, device="cuda")
    t = torch.full((B,), 10, dtype=torch.long, device="cuda")
    a = model(x, t, y=yd)
    assert torch.equal(model(x, t, y=yd), a)
    yd["cmotion"].mul_(0.5)
    assert not torch.equal(model(x, t, y=yd), a)
    with pytest.raises(IndexError):                           # EmbedAction would raise on the table lookup (cmdm.py:363-365)
        model(x, t, y={"cmotion": yd["cmotion"], "action": torch.full((B, 1), cfg["num_actions"], device="cuda")})
    with pytest.raises(IndexError):                           # TimestepEmbedder indexes pe[timesteps] (cmdm.py:298)
        model(x, torch.full((B,), 5000, dtype=torch.long, device="cuda"), y=yd)


def test_model_kwargs_the_fused_loop_does_not_read():
    """y['uncond'] and y['inpainting_mask'/'inpainted_motion'] (gaussian_diffusion.py:319-323, cmdm.py:181) route through
    the per-step API instead of being ignored."""
    from regennet_amd import synth
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    cfg = synth.get_config("tiny")
    sd = synth.make_state_dict(cfg, seed=0)
    model, diffusion = build_hip(cfg, sd, resp="10", precision="bf16x3")
    B, shape = 2, (2, 5, 6, 8)
    tape = torch.from_numpy(synth.make_noise_tape(cfg, B, 10, seed=10))
    y = y_to_device({"cmotion": synth.make_cmotion(cfg, B), "action": synth.make_actions(cfg, B)})
    fused = diffusion.p_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": y}, noise_tape=tape)
    # mask nothing: the per-step path reproduces the fused loop
    none = torch.zeros(shape, dtype=torch.bool, device="cuda")
    target = torch.randn(shape, device="cuda")
    per_step = diffusion.p_sample_loop(model, shape, clip_denoised=False, noise_tape=tape,
                                       model_kwargs={"y": dict(y, inpainting_mask=none, inpainted_motion=target)})
    assert (per_step - fused).abs().max().item() < 1e-4      # same kernels; the per-step API evaluates the timestep MLP per call
    # the same with a SEED instead of a tape: the per-step loop draws the fused loop's own Philox stream (rgn_randn_step), for x_T and
    # for every step, and a motion's draws follow its GLOBAL index (sample_offset), not its place in the call
    fused_s = diffusion.p_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": y}, seed=77, sample_offset=5)
    per_step_s = diffusion.p_sample_loop(model, shape, clip_denoised=False, seed=77, sample_offset=5,
                                         model_kwargs={"y": dict(y, inpainting_mask=none, inpainted_motion=target)})
    assert (per_step_s - fused_s).abs().max().item() < 1e-4 and not torch.allclose(fused_s, fused, atol=1e-2)
    y1 = {k: v[1:] for k, v in y.items()}
    one = diffusion.p_sample_loop(model, (1,) + shape[1:], clip_denoised=False, seed=77, sample_offset=6,
                                  model_kwargs={"y": dict(y1, inpainting_mask=none[1:], inpainted_motion=target[1:])})
    assert (one[0] - per_step_s[1]).abs().max().item() < 1e-4
    eng = model._rgn_bind(B, y)[0]
    z = torch.empty(shape, device="cuda")
    with pytest.raises(RuntimeError):
        eng.randn_step(z, B, 77, 0, -2, 0)                    # loop_index < -1: RGN_ERR_INVALID_ARG
    # mask everything: x_0 is the inpainted motion (coef1[0] = 1, coef2[0] = 0, no noise at t = 0)
    every = torch.ones(shape, dtype=torch.bool, device="cuda")
    forced = diffusion.p_sample_loop(model, shape, clip_denoised=False, noise_tape=tape,
                                     model_kwargs={"y": dict(y, inpainting_mask=every, inpainted_motion=target)})
    assert (forced - target).abs().max().item() < 1e-5
    # half mask: masked entries equal the target, the others differ from the unconstrained sample
    half = torch.zeros(shape, dtype=torch.bool, device="cuda")
    half[..., :4] = True
    mixed = diffusion.p_sample_loop(model, shape, clip_denoised=False, noise_tape=tape,
                                    model_kwargs={"y": dict(y, inpainting_mask=half, inpainted_motion=target)})
    assert (mixed[..., :4] - target[..., :4]).abs().max().item() < 1e-5 and not torch.allclose(mixed[..., 4:], fused[..., 4:])
    # y['uncond'] = True: the unconditional branch only == guidance with scale 0 (out_u + 0 * (out_c - out_u))
    unc = diffusion.p_sample_loop(model, shape, clip_denoised=False, noise_tape=tape, model_kwargs={"y": dict(y, uncond=True)})
    g0 = diffusion.p_sample_loop(ClassifierFreeSampleModel(model), shape, clip_denoised=False, noise_tape=tape,
                                 model_kwargs={"y": dict(y, scale=torch.zeros(B, device="cuda"))})
    assert (unc - g0).abs().max().item() < 1e-4 and not torch.allclose(unc, fused, atol=1e-3)


def test_sequence_length_follows_the_call_like_the_reference():
    """The reference's module is length-agnostic (x.shape[-1], cmdm.py:176): `--motion_length 40` on an NTU model samples
    40 frames (sample/cgenerate.py:40,126). One model object, T = 60 then 40, each against the oracle."""
    from oracle import regennet_oracle as orc
    from regennet_amd import synth
    cfg = synth.get_config("ntu_action", layers=2)
    sd = synth.make_state_dict(cfg, seed=3)
    model, diffusion = build_hip(cfg, sd, resp="ddim5", precision="bf16x3")
    B = 2
    for T in (60, 40, 60):
        cfgT = dict(cfg, num_frames=T)
        y = {"cmotion": synth.make_cmotion(cfgT, B, seed=51), "action": synth.make_actions(cfgT, B, seed=52)}
        tape = synth.make_noise_tape(cfgT, B, 5, seed=53)
        ref = orc.sample_loop(sd, cfgT, orc.make_schedule("cosine", "ddim5"), tape, {k: torch.from_numpy(v) for k, v in y.items()},
                              mode="ddim").numpy()
        out = diffusion.ddim_sample_loop(model, (B, 56, 6, T), clip_denoised=False, model_kwargs={"y": y_to_device(y)},
                                         noise_tape=torch.from_numpy(tape))
        assert np.abs(out.cpu().numpy() - ref).max() < 1e-3, T


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["tiny_opts_clip", "tiny_opts_large_linear", "tiny_opts_skip_init", "tiny_opts_skip_zero",
                                  "tiny_opts_eta"])
def test_sampler_options(golden, name, precision):
    """Options of p_sample_loop / ddim_sample_loop beyond the cgenerate defaults, against the reference:
    clip_denoised=True, FIXED_LARGE variance + linear schedule, skip_timesteps (+ init_image), DDIM eta > 0."""
    from regennet_amd import synth
    g = golden(name)
    cfg, sd, y, tape = fixture_inputs(g, loop=True)
    o = fixture_opts(g)
    model, diffusion = build_hip(cfg, sd, resp=str(g["resp"]), precision=precision,
                                 noise_schedule=o.get("noise_schedule", "cosine"), sigma_small=o.get("sigma_small", True))
    fm = _wrap(model, bool(g["guided"]))
    shape = (int(g["B"]), cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    kw = dict(clip_denoised=o.get("clip_denoised", False), model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape),
              skip_timesteps=o.get("skip_timesteps", 0))
    if o.get("init_image"):
        kw["init_image"] = torch.from_numpy(synth.make_noise_tape(cfg, int(g["B"]), 0, seed=12)[0] * 0.5).cuda()
    if str(g["mode"]) == "ddpm":
        out = diffusion.p_sample_loop(fm, shape, **kw)
    else:
        out = diffusion.ddim_sample_loop(fm, shape, eta=o.get("eta", 0.0), **kw)
    err = np.abs(out.cpu().numpy() - g["final"]).max()
    assert err < 1e-3, (name, err)


# ---- next-3 row: auto_regressive generation (eval/a2m/stgcn_eval.py:50-67) --------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["tiny_autoreg_ddpm10", "tiny_add_autoreg_ddpm20"])
def test_auto_regressive_matches_reference(golden, name, precision):
    """All T runs as one batch (and as several calls) against the reference's frame-by-frame loop on the same noise."""
    from regennet_amd.eval import sample_auto_regressive

    g = golden(name)
    cfg, sd, y, tapes = autoreg_inputs(g)
    model, diffusion = build_hip(cfg, sd, resp=str(g["resp"]), precision=precision)
    B, T = int(g["B"]), int(g["T"])
    shape = (B, cfg["njoints"], cfg["nfeats"], T)
    tapes_t = [torch.from_numpy(t) for t in tapes]
    for fpc, trunc in ((T, True), (3, True), (1, True), (3, False)):   # truncated sequences (frame f needs tokens 0..f only) and full ones
        out = sample_auto_regressive(diffusion.p_sample_loop, model, shape, {"y": y_to_device(y)}, frames_per_call=fpc,
                                     noise_tapes=tapes_t, truncate=trunc)
        err = np.abs(out.cpu().numpy() - g["output"]).max()
        assert err < 1e-3, (name, fpc, trunc, err)


def test_auto_regressive_grouping_invariance_with_device_rng():
    """Philox keyed by the global (frame, sample) index: the grouping of frames into sampler calls cannot change a bit."""
    from regennet_amd import synth
    from regennet_amd.eval import sample_auto_regressive

    cfg = synth.get_config("tiny")
    sd = synth.make_state_dict(cfg, seed=0)
    model, diffusion = build_hip(cfg, sd, resp="10", precision="bf16x3")
    B, T = 3, cfg["num_frames"]
    y = y_to_device({"cmotion": synth.make_cmotion(cfg, B, seed=1), "action": synth.make_actions(cfg, B, seed=2)})
    shape = (B, cfg["njoints"], cfg["nfeats"], T)
    ref = sample_auto_regressive(diffusion.p_sample_loop, model, shape, {"y": y}, frames_per_call=T, seed=11)
    for fpc, trunc in ((1, True), (3, True), (3, False)):    # grouping and sequence truncation: neither changes a bit
        out = sample_auto_regressive(diffusion.p_sample_loop, model, shape, {"y": y}, frames_per_call=fpc, seed=11, truncate=trunc)
        assert torch.equal(out, ref), (fpc, trunc)
    other = sample_auto_regressive(diffusion.p_sample_loop, model, shape, {"y": y}, frames_per_call=T, seed=12)
    assert not torch.equal(other, ref)


@pytest.mark.parametrize("T", [65, 96, 97, 128, 129, 160])
def test_long_sequence_attention_units_against_the_unfused_path(T):
    """k_qkv_attn_long splits the causal attention of a (sample, head) into nine (query tile, key-tile range) units whose partial
    results are merged flash-style; which units see valid keys depends on the length (at <= 128 tokens the unit of query tile 4 has
    none at all). Check every tile-count / remainder combination against the unfused plain-bf16 path (in_proj GEMM + k_attn_x3,
    REGENNET_NO_QKV_LONG=1: same operands, one wave per query tile) on whole sampling runs - a key tile dropped or double-counted
    would show as O(0.1), the two roundings agree to ~1e-3 - and against the oracle within the plain-bf16 phase's own error."""
    import os
    from oracle import regennet_oracle as orc
    from regennet_amd import synth
    cfg = synth.get_config("ntu_action", layers=1, num_frames=T)   # one layer, two steps: rounding differences stay small, a wrong key set does not
    sd = synth.make_state_dict(cfg, seed=3)
    B, S = 3, 2
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=6), "action": synth.make_actions(cfg, B, seed=7)}
    tape = synth.make_noise_tape(cfg, B, S, seed=8)
    outs = []
    for unfused in (False, True):
        if unfused:
            os.environ["REGENNET_NO_QKV_LONG"] = "1"
        try:
            model, diffusion = build_hip(cfg, sd, resp=f"ddim{S}", precision="bf16_x3tail/throughput", x3_tail=0)
            outs.append(diffusion.ddim_sample_loop(model, (B, 56, 6, T), clip_denoised=False, model_kwargs={"y": y_to_device(y)},
                                                   noise_tape=torch.from_numpy(tape)).cpu().numpy())
            model._engine.close()
        finally:
            os.environ.pop("REGENNET_NO_QKV_LONG", None)
    ref = orc.sample_loop(sd, cfg, orc.make_schedule("cosine", f"ddim{S}"), tape, {k: torch.from_numpy(v) for k, v in y.items()},
                          mode="ddim", guided=False).numpy()
    d_paths = float(np.abs(outs[0] - outs[1]).max())
    d_ref, d_ref_unfused = float(np.abs(outs[0] - ref).max()), float(np.abs(outs[1] - ref).max())
    print(f"\n[long attention units] T={T}: fused vs unfused {d_paths:.2e}, vs oracle (plain bf16 throughout): fused {d_ref:.2e}, unfused {d_ref_unfused:.2e}")
    assert np.isfinite(outs[0]).all()
    assert d_ref < 2.0 * d_ref_unfused + 2e-3, (T, d_ref, d_ref_unfused)
    assert d_paths < 2.0 * d_ref_unfused + 2e-3, (T, d_paths, d_ref_unfused)


def test_rccl_one_rank_group_takes_the_multi_gpu_code_paths():
    """utils/dist_util.py:20-83's counterpart on the pool's hardware, every round: a ONE-rank RCCL group (two ranks cannot share a GPU) in a
    subprocess - backend init with the environment bench.py gives its ranks, the start-up broadcast of the checkpoint as one flat fp32 buffer
    (dist_util.sync_model_weights), the MAX all-reduce of the calibration agreement - and `bench.py --force-dist` end to end:
    process-group init, checkpoint broadcast, local engine build, barriers around the timed region, MAX all-reduce of the time."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "rccl_single_rank_check.py")], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "[rccl] ok" in p.stdout and "values unchanged: True" in p.stdout, p.stdout + p.stderr
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29533")
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--force-dist", "--steps", "1", "--warmup", "1", "--respacing", "50", "--batch", "64",
                        "--full", "--no-cpu-baseline", "--profile-evals", "0"], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, p.stdout + p.stderr
    line = json.loads(lines[-1])
    assert line["backend"] == "nccl" and line["rccl_world_size"] == 1 and line["value"] > 0, line
    assert line["headline_row_check_max_abs"] is not None and line["headline_row_check_max_abs"] <= 2e-5, line
    assert 100e6 < line["weights_broadcast_bytes"] < 130e6, line            # the fp32 checkpoint once, not the packed blob


def test_per_handle_kernel_switches():
    """rgn_set_option: the REGENNET_<KEY> switches for ONE handle - unknown names and calls behind rgn_finalize_weights are refused, and a
    handle's option wins over the environment (here: the one-kernel decoder stack switched off for one engine while the environment asks for it)."""
    from regennet_amd import _lib, synth
    cfg = synth.get_config("ntu")
    eng = _lib.Engine(cfg, 64, 0, "bf16_x3tail", options={"LAYERS": 0})
    assert eng.lib.rgn_set_option(eng.h, b"NO_SUCH_SWITCH", 1) == -2
    for k, v in synth.make_state_dict(cfg, seed=0).items():
        eng.load_weight(k, v)
    eng.finalize()
    assert eng.lib.rgn_set_option(eng.h, b"LAYERS", 1) == -5
    assert "layers" not in eng.plan_query(64) and "steps_fused" not in eng.plan_query(64) and "mlp" in eng.plan_query(64)
    eng.close()
    eng2 = _lib.Engine(cfg, 64, 0, "bf16_x3tail")
    for k, v in synth.make_state_dict(cfg, seed=0).items():
        eng2.load_weight(k, v)
    eng2.finalize()
    plan = eng2.plan_query(64)
    assert plan["steps_fused"]["kernel"] == "k_layers<true>" and plan["steps_fused"]["flops"] > 0, plan
    assert eng2.plan_query(8) and "sb_gemm" in eng2.plan_query(8), eng2.plan_query(8)          # 480 token rows: the small-batch engine
    eng2.close()


@pytest.mark.parametrize("cfg_name,B,guided,opts", [("ntu", 64, False, {}), ("ntu", 64, False, {"LAYERS_STEPS": 0}), ("ntu", 64, False, {"LAYERS": 0}),
                                                  ("ntu_action", 64, True, {}), ("ntu_action", 64, True, {"LAYERS_GUIDED": 2}), ("chi3d", 8, False, {}), ("ntu", 4, False, {})])
def test_the_reported_plan_is_what_the_engine_launches(cfg_name, B, guided, opts):
    """rgn_plan_query (what bench.py prices) against rgn_profile_query (what was launched): one eager, profiled, plain-bf16 sampling step per
    configuration - the kernel classes with launches and their launch counts per evaluation must agree with the plan, for the one-kernel stack, its
    per-step form, the kernel-per-stage chain, guidance (an evaluation per workgroup: the engine's choice at 2 B <= #CUs; a motion per workgroup: forced),
    150 frames and the small-batch engine."""
    from regennet_amd import synth
    cfg = synth.get_config(cfg_name)
    sd = synth.make_state_dict(cfg, seed=0)
    model, diffusion = build_hip(cfg, sd, resp="8", precision="bf16_x3tail", x3_tail=0)
    model.engine_options = dict(opts, STREAMS=1)
    eng, dev = model._get_engine(B)
    y = {"cmotion": torch.from_numpy(synth.make_cmotion(cfg, B, seed=1)).cuda()}
    if cfg["cond_mode"] == "action":
        y["action"] = torch.from_numpy(synth.make_actions(cfg, B, seed=2)).cuda()
    if guided:
        y["scale"] = torch.full((B,), 2.5, device="cuda")
    fm = _wrap(model, guided)
    shape = (B, cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    fn = diffusion.ddim_sample_loop if guided else diffusion.p_sample_loop
    fn(fm, shape, clip_denoised=False, model_kwargs={"y": y}, seed=3)                 # binds schedule + condition, warms the kernels
    plan = eng.plan_query(B, guided, split_phase=False)
    st = torch.cuda.current_stream().cuda_stream
    x = torch.empty(shape, device="cuda")
    eng.randn(x, B, 3, 0, st)
    eng.profile_enable(True)
    steps = 3
    eng.sample_range("ddim" if guided else "ddpm", guided, 0.0, x, None, 3, 0, 7, steps, None, False, False, st)
    torch.cuda.synchronize()
    prof = {k: n for k, (ms, n) in eng.profile_query().items() if n > 0}
    eng.profile_enable(False)
    launched = {k: n for k, n in prof.items() if k not in ("embed", "misc")}             # (once-per-call work in front of the first fused step)
    for cls, rec in plan.items():
        if cls == "steps_fused":
            assert launched.get(cls) == 1, (cls, launched, plan)                         # ONE launch for the whole run of steps
        elif rec["launches_per_eval"] > 0:
            want = rec["launches_per_eval"] * steps
            got = launched.get(cls, 0)
            if cls in ("gemm_mfma", "update", "sb_gemm"):    # + once per call: the state pack (k_pack_x) / the up-front embedding in front of the first step
                assert want <= got <= want + 1, (cls, got, want, launched, plan)
            else:
                assert got == want, (cls, got, want, launched, plan)
    for cls, n in launched.items():
        assert cls in plan or (cls in ("gemm_mfma", "update") and n == 1), (cls, launched, plan)
    model._engine.close()


def test_exceptions_do_not_cross_the_c_boundary():
    """include/regennet_hip.h: "no exceptions cross the boundary". A positional table of 2^40 rows (its first dimension is free) makes the
    host-side copy throw std::length_error / std::bad_alloc inside rgn_load_weight: it must come back as RGN_ERR_INTERNAL with the text in
    rgn_last_error - not unwind into ctypes - and the handle stays usable."""
    import ctypes as C
    from regennet_amd import _lib, synth
    cfg = synth.get_config("tiny")
    eng = _lib.Engine(cfg, 1, 0, "f32")
    host = np.zeros(16, np.float32)
    shape = (C.c_int64 * 3)(1 << 40, 1, cfg["latent_dim"])
    code = eng.lib.rgn_load_weight(eng.h, b"sequence_pos_encoder.pe", host.ctypes.data_as(C.c_void_p), shape, 3)
    assert code == -8, code
    msg = eng.lib.rgn_last_error(eng.h).decode()
    assert "rgn_load_weight" in msg and "exception" in msg, msg
    for k, v in synth.make_state_dict(cfg, seed=0).items():      # the handle is intact: a checkpoint still loads and finalizes
        eng.load_weight(k, v)
    eng.finalize()
    eng.close()
