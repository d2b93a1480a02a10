"""GPU: arch='gru' (the reference's nn.GRU denoiser, model/cmdm.py:191-199, 243-249; rgn_gru_stack.hip) against goldens recorded from the reference
(tests/golden/make_golden_gru_arch.py) in both scans and every precision mode: forward and sampling-loop parity, what the two scans couple and what
they do not (bit for bit), graph replay, the plan the engine reports, and the refusals."""
import os

import numpy as np
import pytest
import torch

from regennet_amd import _lib, synth
from tests.gru_arch_cases import FORWARD, LOOPS, inpaint_inputs
from tests.helpers import build_hip, fixture_inputs, y_to_device

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PRECISIONS = ["f32", "bf16x3", "bf16_x3tail"]
TOL = {"f32": 2e-4, "bf16x3": 1e-3, "bf16_x3tail": 1e-3}     # the bounds tests/test_mlp_arch_gpu.py holds the other architectures to


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


def _build(cfg, sd, scan, **kw):
    model, diffusion = build_hip(cfg, sd, **kw)
    model.gru_scan = scan
    return model, diffusion


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", sorted(FORWARD))
def test_gru_forward_goldens(name, precision):
    """Every recorded timestep (0 and 999 among them), the y['uncond'] rows, and one rgn_denoise call with a different timestep per sample."""
    g = _golden(name)
    cfg, sd, y, x = fixture_inputs(g, loop=False)
    scan, guided = str(g["scan"]), bool(g["guided"])
    model, _ = _build(cfg, sd, scan, precision=precision)
    fm = _wrap(model, guided)
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
    plan = model._engine.plan_query(B, guided=guided, split_phase=True)
    _close(model)
    print(f"\n[gru forward err] {name} {precision}: {errs}")
    st = plan["gru_stack"]
    S = B if scan == "batch" else cfg["num_frames"]
    assert st["kernel"] == f"k_gru_stack<{scan}>" and st["scan"] == scan and st["steps"] == S and st["launches_per_eval"] == S + cfg["layers"] - 1, plan
    assert st["segments"] == (2 if guided and scan == "batch" else 1) and st["workspace_bytes"] > 0, plan
    assert not any(k in plan for k in ("layers", "steps_fused", "step_fused", "sb_gemm", "attention", "qkv_attn", "mlp", "mixer")), plan
    assert max(errs.values()) < TOL[precision], (name, precision, errs)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", sorted(LOOPS))
def test_gru_sampling_loop_goldens(name, precision):
    g = _golden(name)
    cfg, sd, y, tape = fixture_inputs(g, loop=True)
    if LOOPS[name][5]:
        mask, target = inpaint_inputs(cfg, int(g["B"]))
        y = dict(y, inpainting_mask=mask, inpainted_motion=target)
    model, diffusion = _build(cfg, sd, str(g["scan"]), resp=str(g["resp"]), precision=precision)
    shape = (int(g["B"]), cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    fn = diffusion.p_sample_loop if str(g["mode"]) == "ddpm" else diffusion.ddim_sample_loop
    out = fn(_wrap(model, bool(g["guided"])), shape, clip_denoised=False, model_kwargs={"y": y_to_device(y)}, noise_tape=torch.from_numpy(tape)).cpu().numpy()
    f16, tail = model._engine.precision_plan(int(g["B"]), bool(g["guided"]))
    _close(model)
    err = float(np.abs(out - g["final"]).max())
    print(f"\n[gru loop err] {name} {precision}: {err:.2e}")
    assert f16 == 0 and (precision == "f32" or tail == int(g["S"])), (f16, tail)      # split-bf16 on every step by default, never an fp16 sub-phase
    assert err < TOL[precision], (name, precision, err)


# ---- what the scans couple: bit for bit, what a tolerance hides (indexing, in-place and ring mistakes)
def _case(B, frames=19):
    cfg = synth.get_config("tiny_gru", num_frames=frames)           # 19 frames / 5 samples: a ragged second group of sequences in either scan
    sd = synth.make_state_dict(cfg, seed=0)
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=1), "action": synth.make_actions(cfg, B, seed=2)}
    x = synth.make_noise_tape(cfg, B, 0, seed=11)[0]
    return cfg, sd, y, x


def _fwd(model, x, y, t=400):
    B = x.shape[0]
    return model(torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.full((B,), t, dtype=torch.long, device="cuda"),
                 y=y_to_device({k: np.ascontiguousarray(v) for k, v in y.items()})).cpu().numpy()


@pytest.mark.parametrize("precision", ["f32", "bf16_x3tail"])
def test_batch_scan_prefix_and_frame_independence_bit_for_bit(precision):
    """The first k samples of a batch of B equal a batch of those k alone; changing one frame of sample 1 changes that frame of samples 1 .. B - 1
    and no other frame of any sample."""
    B = 5
    cfg, sd, y, x = _case(B)
    model, _ = _build(cfg, sd, "batch", precision=precision)
    full = _fwd(model, x, y)
    for k in (1, 3):
        part = _fwd(model, x[:k], {n: v[:k] for n, v in y.items()})
        assert np.array_equal(part, full[:k]), k
    x2 = x.copy()
    x2[1, :, :, 7] += 0.5
    moved = _fwd(model, x2, y)
    _close(model)
    changed = (moved != full).any(axis=(1, 2))                       # [B, T]
    want = np.zeros_like(changed)
    want[1:, 7] = True
    assert np.array_equal(changed, want), changed


@pytest.mark.parametrize("precision", ["f32", "bf16_x3tail"])
def test_frames_scan_sample_alone_equals_batched_and_permuted_bit_for_bit(precision):
    B = 5
    cfg, sd, y, x = _case(B)
    model, _ = _build(cfg, sd, "frames", precision=precision)
    full = _fwd(model, x, y)
    perm = np.array([3, 0, 4, 2, 1])
    shuffled = _fwd(model, x[perm], {n: v[perm] for n, v in y.items()})
    assert np.array_equal(shuffled, full[perm])
    for b in (0, 4):
        one = _fwd(model, x[b:b + 1], {n: v[b:b + 1] for n, v in y.items()})
        assert np.array_equal(one[0], full[b]), b
    _close(model)


@pytest.mark.parametrize("scan", ["batch", "frames"])
def test_graph_replay_equals_eager_launches_and_streams_do_not_matter(scan):
    """Guided DDPM, 10 steps: captured graphs against eager launches, and STREAMS = 4 against 1 (the stack runs on one chain whatever it says)."""
    B, S = 3, 10
    cfg = synth.get_config("tiny_gru")
    sd = synth.make_state_dict(cfg, seed=0)
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=1), "action": synth.make_actions(cfg, B, seed=2), "scale": np.full((B,), 2.5, dtype=np.float32)}
    tape = synth.make_noise_tape(cfg, B, S, seed=10)
    outs = []
    for streams, graph in ((4, True), (4, False), (1, True)):
        model, diffusion = _build(cfg, sd, scan, resp=str(S), precision="bf16_x3tail", engine_options={"STREAMS": streams})
        outs.append(diffusion.p_sample_loop(_wrap(model, True), tape.shape[1:], clip_denoised=False, model_kwargs={"y": y_to_device(y)},
                                            noise_tape=torch.from_numpy(tape), use_graph=graph).cpu().numpy())
        _close(model)
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


def test_the_scan_is_a_property_of_the_model_and_switches_between_calls():
    B = 3
    cfg, sd, y, x = _case(B, frames=8)
    model, _ = _build(cfg, sd, "batch")
    a = _fwd(model, x, y)
    model.gru_scan = "frames"
    b = _fwd(model, x, y)
    model.gru_scan = "batch"
    c = _fwd(model, x, y)
    info = model._engine.gru_stack_info(B)
    _close(model)
    assert np.array_equal(a, c) and np.abs(a - b).max() > 1e-2                  # two different functions of the same weights
    assert (info["scan"], info["segments"], info["steps"], info["launches_per_eval"]) == ("batch", 1, B, B + cfg["layers"] - 1), info


# ---- refusals
def _engine(cfg, options=None, precision="f32"):
    sd = synth.make_state_dict(cfg, seed=0)
    eng = _lib.Engine(dict(cfg), 2, 0, precision, **({"options": options} if options else {}))
    try:
        for k, v in sd.items():
            eng.load_weight(k, v)
        eng.finalize()
    except BaseException:
        eng.close()
        raise
    return eng


@pytest.mark.parametrize("key", ["LAYERS", "LAYERS_STEPS", "LAYERS_MIN_B", "LAYERS_GUIDED"])
def test_refuses_the_layers_switches(key):
    with pytest.raises(_lib.RgnError, match=r"UNSUPPORTED.*LAYERS.*arch='gru'"):
        _engine(synth.get_config("tiny_gru"), options={key: 1})


@pytest.mark.parametrize("key", ["NO_STEP_FUSION", "STEP_NO_QUADS"])
def test_refuses_the_step_boundary_switches(key):
    with pytest.raises(_lib.RgnError, match=r"UNSUPPORTED.*k_step.*arch='gru'"):
        _engine(synth.get_config("tiny_gru"), options={key: 1})


def test_small_batch_engine_fp16_phase_and_scan_setter_refusals():
    eng = _engine(synth.get_config("ntu_gru", layers=1), precision="bf16_x3tail")
    try:
        plan = eng.plan_query(1)
        assert "sb_gemm" not in plan and "gru_stack" in plan                      # 60 token rows: where a transformer handle takes the small-batch engine
        eng.set_small_batch_rows(0)
        eng.set_small_batch_rows(-1)
        with pytest.raises(_lib.RgnError, match=r"UNSUPPORTED.*small-batch.*arch='gru'"):
            eng.set_small_batch_rows(640)
        with pytest.raises(_lib.RgnError, match=r"INVALID_ARG.*scan"):
            eng.set_gru_scan(2)
        eng.set_gru_scan("frames")
        assert eng.plan_query(1)["gru_stack"]["kernel"] == "k_gru_stack<frames>"
    finally:
        eng.close()
    other = _engine(synth.get_config("tiny_add"))
    try:
        with pytest.raises(_lib.RgnError, match=r"UNSUPPORTED.*not 'gru'"):
            other.set_gru_scan("frames")
        with pytest.raises(_lib.RgnError, match=r"UNSUPPORTED.*not 'gru'"):
            other.gru_stack_info(1)
    finally:
        other.close()


def test_refuses_a_concat_checkpoint_and_wrong_shapes():
    cfg = synth.get_config("tiny_gru")
    with pytest.raises(_lib.RgnError, match=r"UNSUPPORTED.*cm_mode add"):
        _lib.Engine(dict(cfg, layers=cfg["layers"], cm_mode="concat"), 2, 0, "f32")
    sd = synth.make_state_dict(cfg, seed=0)
    eng = _lib.Engine(dict(cfg), 2, 0, "f32")
    try:
        with pytest.raises(_lib.RgnError, match=r"BAD_SHAPE.*input_process"):
            eng.load_weight("input_process.poseEmbedding.weight", sd["input_process.poseEmbedding.weight"][:, :30])   # [d, F] where the gru model holds [d, F + d]
        with pytest.raises(_lib.RgnError, match=r"BAD_KEY.*fuse_process"):
            eng.load_weight("fuse_process.weight", np.zeros((64, 128), dtype=np.float32))
        for k, v in sd.items():
            if k != "gru.bias_hh_l1":
                eng.load_weight(k, v)
        with pytest.raises(_lib.RgnError, match=r"MISSING_KEY.*gru\.bias_hh_l1"):
            eng.finalize()
    finally:
        eng.close()
