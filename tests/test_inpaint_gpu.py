"""GPU: motion in-painting inside the fused sampling loop (rgn_set_inpainting; gaussian_diffusion.py:319-323) against the reference's
own runs (tests/golden/inpaint_*.npz, recorded by tests/golden/make_golden_inpaint.py), in every precision mode and on every form of
the step boundary the engine dispatches: k_update, k_step, k_layers<true> - unguided, guided, fp16 phase."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from regennet_amd import synth
from regennet_amd._lib import RgnError
from tests.helpers import build_hip, fixture_inputs, y_to_device
from tests.inpaint_cases import CASES, case_inputs
from tests.test_offline_gpu import PRECISIONS, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

FORMS = [(name, p, None) for name in sorted(CASES) for p in PRECISIONS]
for _n in ("inpaint_ntu_ddpm50_b64", "inpaint_ntu_action_ddim5_cfg_b64"):
    FORMS += [(_n, "bf16_x3tail", {"LAYERS": 0}), (_n, "bf16_x3tail", {"LAYERS_STEPS": 0}), (_n, "bf16_x3tail", {"NO_STEP_FUSION": 1})]
FORMS += [("inpaint_ntu_action_ddim5_cfg_b64", "bf16_x3tail", {"LAYERS_GUIDED": 0}), ("inpaint_ntu_action_ddim5_cfg_b64", "bf16_x3tail", {"LAYERS_GUIDED": 2})]


def _golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _wrap(model, guided):
    if not guided:
        return model
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    return ClassifierFreeSampleModel(model)


def _setup(name, precision, opts=None, **kw):
    g = _golden(name)
    cfg, sd, y, tape = fixture_inputs(g, loop=True)
    case, _, mask, target = case_inputs(name)
    model, diffusion = build_hip(cfg, sd, resp=str(g["resp"]), precision=precision, engine_options=opts, **kw)
    fm = _wrap(model, bool(g["guided"]))
    shape = (int(g["B"]), cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    fn = diffusion.p_sample_loop if str(g["mode"]) == "ddpm" else diffusion.ddim_sample_loop
    base = dict(clip_denoised=bool(g["clip"]), noise_tape=torch.from_numpy(tape))
    return g, y_to_device(y), mask, target, model, diffusion, fm, shape, fn, base


def _inp(yd, mask, target):
    return {"y": dict(yd, inpainting_mask=torch.from_numpy(mask).cuda(), inpainted_motion=torch.from_numpy(target).cuda())}


@pytest.mark.parametrize("name,precision,opts", FORMS)
def test_inpaint_goldens_and_exactness(name, precision, opts):
    """The reference's result within the precision mode's bound; masked elements equal the target bit for bit; an all-False mask gives the
    bits of the call without a mask; an all-True mask gives the target bit for bit."""
    if "/" in precision and "tiny" in name:
        pytest.skip("the small-batch engine only takes d = 512 models: same kernels as the plain mode")
    g, yd, mask, target, model, diffusion, fm, shape, fn, base = _setup(name, precision, opts)
    out = fn(fm, shape, model_kwargs=_inp(yd, mask, target), **base).cpu().numpy()
    want = np.clip(target, -1, 1) if bool(g["clip"]) else target
    ref, got = (g["final_rows"], out[g["rows"]]) if "rows" in g else (g["final"], out)
    err = float(np.abs(got - ref).max())
    print(f"\n[inpaint loop err] {name} {precision} {opts}: {err:.2e}")
    assert err < TOL[precision], (name, precision, opts, err)
    assert np.array_equal(out[mask], want[mask]), "masked elements are the target, bit for bit"
    plain = fn(fm, shape, model_kwargs={"y": yd}, **base).cpu().numpy()
    none = fn(fm, shape, model_kwargs=_inp(yd, np.zeros_like(mask), target), **base).cpu().numpy()
    assert np.array_equal(none, plain), "an all-False mask changes nothing"
    every = fn(fm, shape, model_kwargs=_inp(yd, np.ones_like(mask), target), **base).cpu().numpy()
    assert np.array_equal(every, want), "an all-True mask returns the target"


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_inpaint_trace_per_step(precision):
    """Every step's sample and pred_xstart of the traced fixture, through the progressive generator."""
    g, yd, mask, target, model, diffusion, fm, shape, fn, base = _setup("inpaint_tiny_ddpm10", precision)
    steps = list(diffusion.p_sample_loop_progressive(fm, shape, model_kwargs=_inp(yd, mask, target), **base))
    assert len(steps) == int(g["S"])
    for k, out in enumerate(steps):
        ex = float((out["sample"].cpu().numpy() - g["x"][k]).__abs__().max())
        e0 = float((out["pred_xstart"].cpu().numpy() - g["x0"][k]).__abs__().max())
        assert ex < TOL[precision] and e0 < TOL[precision], (k, ex, e0)
        assert np.array_equal(out["pred_xstart"].cpu().numpy()[mask], target[mask]), k      # the yielded pred_xstart is the blended one


def test_fused_path_is_taken(monkeypatch):
    """With _loop_per_step patched to raise, both samplers complete with both keys; a B = 64 call reports launches of the k_layers<true> class."""
    from regennet_amd.diffusion.gaussian_diffusion import GaussianDiffusion

    def boom(*a, **k):
        raise AssertionError("the per-step path was taken")

    monkeypatch.setattr(GaussianDiffusion, "_loop_per_step", boom)
    g, yd, mask, target, model, diffusion, fm, shape, fn, base = _setup("inpaint_tiny_ddpm10", "bf16x3")
    kw = _inp(yd, mask, target)
    assert torch.isfinite(diffusion.p_sample_loop(fm, shape, model_kwargs=kw, **base)).all()
    assert torch.isfinite(diffusion.ddim_sample_loop(fm, shape, model_kwargs=kw, **base)).all()
    g, yd, mask, target, model, diffusion, fm, shape, fn, base = _setup("inpaint_ntu_ddpm50_b64", "bf16_x3tail")
    fn(fm, shape, model_kwargs={"y": yd}, **base)                  # (builds the engine)
    eng = model._engine
    eng.profile_enable(True)
    out = fn(fm, shape, model_kwargs=_inp(yd, mask, target), **base)
    torch.cuda.synchronize()
    prof = eng.profile_query()
    eng.profile_enable(False)
    assert prof.get("steps_fused", (0, 0))[1] >= 1, prof
    assert np.array_equal(out.cpu().numpy()[mask], target[mask])


@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_fused_against_manual_per_step_loop(sampler):
    """A shape with no fixture (ntu, B = 3, 20 steps, bf16x3): the fused loop against the reference's loop structure written out around
    diffusion.p_sample / ddim_sample with the same tape (1e-4: test_model_kwargs_the_fused_loop_does_not_read's bound for this comparison)."""
    cfg = synth.get_config("ntu")
    sd = synth.make_state_dict(cfg, seed=0)
    B, S = 3, 20
    model, diffusion = build_hip(cfg, sd, resp="20" if sampler == "ddpm" else "ddim20", precision="bf16x3")
    shape = (B, cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    tape = torch.from_numpy(synth.make_noise_tape(cfg, B, S, seed=31)).cuda()
    yd = y_to_device({"cmotion": synth.make_cmotion(cfg, B, seed=7)})
    mask = torch.from_numpy(np.random.RandomState(5).rand(*shape) < 0.3).cuda()
    target = torch.from_numpy(synth.make_noise_tape(cfg, B, 0, seed=32)[0] * np.float32(0.5)).cuda()
    kw = {"y": dict(yd, inpainting_mask=mask, inpainted_motion=target)}
    fn = diffusion.p_sample_loop if sampler == "ddpm" else diffusion.ddim_sample_loop
    fused = fn(model, shape, clip_denoised=False, model_kwargs=kw, noise_tape=tape)
    x = tape[0].clone()
    step = diffusion.p_sample if sampler == "ddpm" else diffusion.ddim_sample
    for k, i in enumerate(range(S - 1, -1, -1)):
        x = step(model, x, torch.full((B,), i, device="cuda"), clip_denoised=False, model_kwargs=kw, _noise=tape[1 + k])["sample"]
    err = float((fused - x).abs().max())
    print(f"\n[fused vs manual loop] {sampler}: {err:.2e}")
    assert err < 1e-4, err


def test_rebinding_under_cached_graphs():
    """Mask A, mask B, no mask on one model (cached graphs): each equals what a fresh model gives for that call alone; eager equals graph."""
    name = "inpaint_ntu_ddpm50"
    g, yd, mask, target, model, diffusion, fm, shape, fn, base = _setup(name, "bf16_x3tail/throughput")
    mask_b = np.ascontiguousarray(~mask)
    calls = [_inp(yd, mask, target), _inp(yd, mask_b, target), {"y": yd}]
    got = [fn(fm, shape, model_kwargs=kw, **base).cpu().numpy() for kw in calls]
    eager = [fn(fm, shape, model_kwargs=kw, use_graph=False, **base).cpu().numpy() for kw in calls]
    for i, kw in enumerate(calls):
        _, _, _, _, m2, d2, fm2, _, fn2, _ = _setup(name, "bf16_x3tail/throughput")
        fresh = fn2(fm2, shape, model_kwargs=kw, **base).cpu().numpy()
        assert np.array_equal(got[i], fresh), i
        assert np.array_equal(eager[i], got[i]), i
        m2._engine.close()


def test_rows_equal_single_sample_runs():
    """A motion sampled alone (layers_min_b = 1) equals its row of the B = 64 call with per-sample masks, bit for bit; same with a seed and
    sample_offset."""
    name = "inpaint_ntu_ddpm50_b64"
    g, yd, mask, target, model, diffusion, fm, shape, fn, base = _setup(name, "bf16_x3tail")
    full = fn(fm, shape, model_kwargs=_inp(yd, mask, target), **base).cpu().numpy()
    full_s = fn(fm, shape, model_kwargs=_inp(yd, mask, target), clip_denoised=False, seed=5, sample_offset=100).cpu().numpy()
    cfg, sd, _, tape = fixture_inputs(g, loop=True)
    one_m, one_d = build_hip(cfg, sd, resp=str(g["resp"]), precision="bf16_x3tail/throughput")
    one_m.layers_min_b = 1
    for b in (1, 42):
        y1 = {k: v[b:b + 1] for k, v in yd.items()}
        kw = _inp(y1, mask[b:b + 1], target[b:b + 1])
        one = one_d.p_sample_loop(one_m, (1,) + shape[1:], clip_denoised=False, model_kwargs=kw, noise_tape=torch.from_numpy(tape[:, b:b + 1])).cpu().numpy()
        assert np.array_equal(one[0], full[b]), b
        one = one_d.p_sample_loop(one_m, (1,) + shape[1:], clip_denoised=False, model_kwargs=kw, seed=5, sample_offset=100 + b).cpu().numpy()
        assert np.array_equal(one[0], full_s[b]), b


def test_errors_and_no_leak(monkeypatch):
    g, yd, mask, target, model, diffusion, fm, shape, fn, base = _setup("inpaint_ntu_ddpm50", "bf16_x3tail/throughput")
    plain = fn(fm, shape, model_kwargs={"y": yd}, **base).cpu().numpy()
    tm, tt = torch.from_numpy(mask).cuda(), torch.from_numpy(target).cuda()
    with pytest.raises(TypeError):
        fn(fm, shape, model_kwargs={"y": dict(yd, inpainting_mask=tm.to(torch.uint8), inpainted_motion=tt)}, **base)
    with pytest.raises(AssertionError):
        fn(fm, shape, model_kwargs={"y": dict(yd, inpainting_mask=tm[:1], inpainted_motion=tt[:1])}, **base)
    eng = model._engine
    eng.set_inpainting(tm[:1].contiguous(), tt[:1].contiguous(), 0)          # a binding of 1 motion under a condition of 2
    x = torch.from_numpy(base["noise_tape"][0].numpy()).cuda().contiguous()
    with pytest.raises(RgnError, match=r"holds 1 motions.*condition 2") as ei:
        eng.sample_range("ddpm", False, 0.0, x, None, 1, 0, int(g["S"]) - 1, 1, None, True, False, 0)
    assert ei.value.code == -5
    assert eng.lib.rgn_set_inpainting(eng.h, 1, tm.data_ptr(), None, None) == -1          # exactly one NULL pointer
    assert eng.lib.rgn_set_inpainting(eng.h, 0, tm.data_ptr(), tt.data_ptr(), None) == -1    # B outside (0, max_batch]
    eng.clear_inpainting()
    # a call that raises mid-loop leaves nothing bound: the third sample_range of a progressive run fails
    real, seen = type(eng).sample_range, []

    def failing(self, *a, **k):
        seen.append(1)
        if len(seen) == 3:
            raise RuntimeError("injected")
        return real(self, *a, **k)

    monkeypatch.setattr(type(eng), "sample_range", failing)
    with pytest.raises(RuntimeError, match="injected"):
        list(diffusion.p_sample_loop_progressive(fm, shape, model_kwargs=_inp(yd, mask, target), **base))
    monkeypatch.undo()
    again = fn(fm, shape, model_kwargs={"y": yd}, **base).cpu().numpy()
    assert np.array_equal(again, plain)
    # ... and nothing stays bound between the yields of a progressive generator: a plain call made meanwhile on the same engine is plain
    g, yd, mask, target, model, diffusion, fm, shape, fn, base = _setup("inpaint_ntu_ddpm50", "bf16x3/throughput")
    plain = fn(fm, shape, model_kwargs={"y": yd}, **base).cpu().numpy()
    gen = diffusion.p_sample_loop_progressive(fm, shape, model_kwargs=_inp(yd, mask, target), **base)
    next(gen)
    meanwhile = fn(fm, shape, model_kwargs={"y": yd}, **base).cpu().numpy()
    rest = [out["sample"] for out in gen]
    assert np.array_equal(meanwhile, plain)
    assert np.array_equal(rest[-1].cpu().numpy()[mask], target[mask])


def test_edit_cli_subprocess(tmp_path):
    out = str(tmp_path / "edit")
    r = subprocess.run([sys.executable, "-m", "regennet_amd.sample.edit", "--synthetic", "--num_samples", "8", "--edit_mode", "in_between",
                        "--num_repetitions", "1", "--timestep_respacing", "20", "--output_dir", out], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = np.load(os.path.join(out, "results.npy"), allow_pickle=True).item()
    m = res["mask"]
    assert res["output"].shape == res["input_motions"].shape == m.shape == (8, 56, 6, 60) and m.dtype == bool
    assert m[..., :15].all() and m[..., 45:].all() and not m[..., 15:45].any()
    assert np.array_equal(res["output"][m], res["input_motions"][m])
    assert not np.array_equal(res["output"][~m], res["input_motions"][~m])
