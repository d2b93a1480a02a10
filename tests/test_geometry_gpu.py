"""GPU: every model geometry rgn_create accepts, not only the presets - head counts, head dims, ff widths, feature widths, sequence
lengths, conditioning widths and depths on each side of the shape predicates that pick the kernels (rgn_pack.cpp / rgn_plan.cpp), each
against the oracle on the same noise (the oracle itself is pinned to the reference at these geometries: tests/test_oracle_golden.py "geo_*").

Every case first asserts, through rgn_plan_query, that the kernel form it is meant to exercise is the one planned, then checks
  * uniform split-bf16 ("bf16x3") against the oracle: the project's parity bound, 1e-3 abs (include/regennet_hip.h);
  * the precision schedule with a forced tail (plain-bf16 steps first, split-bf16 steps last): no invented number - the same case in
    precision="bf16" (the same operand rounding on the generic tiles) is the yardstick, bound 2 x yardstick + 2e-3, the rule of
    test_long_sequence_attention_units_against_the_unfused_path: a dropped tile or column shows as O(0.1), two roundings differ at ~1e-3;
  * row consistency (tests/fuzz_cases.py, part 2): a sample of the batch against the same sample drawn alone with the same Philox key -
    bit-identical in the small-batch engine, <= 5e-5 on the throughput kernels: an indexing mistake, not rounding.
Every measured error is printed; profiles/geometry_parity.txt keeps the table."""
import functools

import numpy as np
import pytest
import torch

from tests import geometry_cases as gc
from tests.helpers import build_hip, y_to_device

pytestmark = pytest.mark.gpu

BOUND = 1e-3          # include/regennet_hip.h: parity bound of uniform split-bf16 / fp32 against the oracle
ROW_TOL = 5e-5        # tests/fuzz_cases.py: a sample in the batch vs alone, throughput kernels


def _tag(over):
    return "-".join(f"{k}={v}" for k, v in over.items()) or "preset"


class Case:
    """One geometry + inputs: ntu_action with overrides, B motions, an S-step schedule, recorded noise."""

    def __init__(self, over, B, S=6, sampler="ddim", guided=False, seed=0):
        from regennet_amd import synth
        self.over, self.B, self.S, self.sampler, self.guided, self.seed = dict(over), B, S, sampler, guided, seed
        self.cfg = cfg = synth.get_config("ntu_action", **dict(dict(layers=1), **over))
        self.sd = synth.make_state_dict(cfg, seed=40 + seed)
        self.resp = f"ddim{S}" if sampler == "ddim" else str(S)
        self.shape = (B, cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
        self.y = self.make_y(seed)
        self.tape = synth.make_noise_tape(cfg, B, S, seed=seed + 3)

    def make_y(self, seed):
        from regennet_amd import synth
        cfg, B = self.cfg, self.B
        y = {"cmotion": synth.make_cmotion(cfg, B, seed=seed + 1)}
        if cfg["cond_mode"] == "action":
            y["action"] = synth.make_actions(cfg, B, seed=seed + 2)
        if cfg["cond_mode"] == "text":
            y["text_features"] = synth.make_text_features(cfg, B, seed=seed + 2)
        if self.guided:
            y["scale"] = np.linspace(1.0, 2.5, B).astype(np.float32)       # (<= 2.5: tests/fuzz_cases.py on what larger scales amplify)
        return y

    def oracle(self, y=None, tape=None):
        from oracle import regennet_oracle as orc
        y, tape = self.y if y is None else y, self.tape if tape is None else tape
        return orc.sample_loop(self.sd, self.cfg, orc.make_schedule("cosine", self.resp), tape, {k: torch.from_numpy(v) for k, v in y.items()},
                               mode=self.sampler, guided=self.guided).numpy()

    @functools.cached_property
    def ref(self):
        return self.oracle()

    def build(self, precision, x3_tail=None, **attrs):
        model, diffusion = build_hip(self.cfg, self.sd, resp=self.resp, precision=precision, x3_tail=x3_tail, f16_steps=attrs.pop("f16_steps", None))
        for k, v in attrs.items():
            setattr(model, k, v)
        return model, diffusion

    def sample(self, model, diffusion, y=None, tape=None, shape=None, **kw):
        from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
        fm = ClassifierFreeSampleModel(model) if self.guided else model
        fn = diffusion.p_sample_loop if self.sampler == "ddpm" else diffusion.ddim_sample_loop
        if "seed" not in kw:
            kw["noise_tape"] = torch.from_numpy(self.tape if tape is None else tape)
        try:
            out = fn(fm, shape or self.shape, clip_denoised=False, model_kwargs={"y": y_to_device(self.y if y is None else y)}, **kw)
            torch.cuda.synchronize()
        except Exception as e:   # a GPU fault is a finding: nothing more runs on the card in this session
            if any(s in str(e) for s in ("illegal memory access", "unspecified launch failure", "hardware exception", "HSA_STATUS_ERROR")):
                pytest.exit(f"GPU fault in {_tag(self.over)}: {e}", returncode=3)
            raise
        return out

    def kernels(self, model, split):
        """Kernel names rgn_plan_query reports for one evaluation of this batch in the split-bf16 / the plain phase."""
        eng, _ = model._get_engine(self.B, self.cfg["num_frames"])
        return {rec["kernel"] for cls, rec in eng.plan_query(self.B, self.guided, split_phase=split).items()
                if rec["launches_per_eval"] > 0 or cls == "steps_fused"}        # (steps_fused: one launch per run of steps, none per evaluation)


def _close(model):
    for e in list(model._engines.values()):
        e.close()
    model._engines.clear()
    model._engine = None


def _check_plan(names, want=(), never=()):
    for k in want:
        assert k in names, (k, sorted(names))
    for k in never:
        assert k not in names, (k, sorted(names))


def _x3(case, label, engine="throughput", want=(), never=(), calls=1):
    """Uniform split-bf16 against the oracle (1e-3). calls = 2: a second sampling call on the same handle with other inputs - a kernel that
    dirtied K-padding columns in the first shows in the second."""
    model, diffusion = case.build("bf16x3" + ("/throughput" if engine == "throughput" else ""))
    _check_plan(case.kernels(model, True), want, never)
    errs = [float(np.abs(case.sample(model, diffusion).cpu().numpy() - case.ref).max())]
    if calls == 2:
        from regennet_amd import synth
        y2, tape2 = case.make_y(case.seed + 50), synth.make_noise_tape(case.cfg, case.B, case.S, seed=case.seed + 53)
        errs.append(float(np.abs(case.sample(model, diffusion, y=y2, tape=tape2).cpu().numpy() - case.oracle(y2, tape2)).max()))
    _close(model)
    print(f"\n[geometry] {label} {_tag(case.over)} B={case.B} T={case.cfg['num_frames']} bf16x3/{engine}: vs oracle " + " / ".join(f"{e:.2e}" for e in errs))
    for e in errs:
        assert e < BOUND, (label, case.over, errs)
    return errs


def _f32(case, label, want=(), never=()):
    """precision f32 against the oracle (1e-3), after the plan names what it should."""
    model, diffusion = case.build("f32")
    _check_plan(case.kernels(model, True), want, never)
    err = float(np.abs(case.sample(model, diffusion).cpu().numpy() - case.ref).max())
    _close(model)
    print(f"\n[geometry] {label} {_tag(case.over)} B={case.B} T={case.cfg['num_frames']} f32: vs oracle {err:.2e}")
    assert err < BOUND, (label, case.over, err)
    return err


def _sched(case, label, tail, want_plain=(), want_split=(), never_plain=(), calls=1, **attrs):
    """The precision schedule with `tail` split-bf16 steps behind S - tail plain-bf16 ones (throughput kernels), against the oracle, bounded by
    twice the error of precision="bf16" on the same case + 2e-3."""
    from regennet_amd import synth
    model, diffusion = case.build("bf16_x3tail/throughput", x3_tail=tail, **attrs)
    _check_plan(case.kernels(model, False), want_plain, never_plain)
    _check_plan(case.kernels(model, True), want_split)
    inputs = [(None, None)]
    if calls == 2:
        inputs.append((case.make_y(case.seed + 50), synth.make_noise_tape(case.cfg, case.B, case.S, seed=case.seed + 53)))
    refs = [case.ref] + [case.oracle(y, t) for y, t in inputs[1:]]
    errs = [float(np.abs(case.sample(model, diffusion, y=y, tape=t).cpu().numpy() - r).max()) for (y, t), r in zip(inputs, refs)]
    _close(model)
    model, diffusion = case.build("bf16/throughput")
    yard = [float(np.abs(case.sample(model, diffusion, y=y, tape=t).cpu().numpy() - r).max()) for (y, t), r in zip(inputs, refs)]
    _close(model)
    print(f"\n[geometry] {label} {_tag(case.over)} B={case.B} T={case.cfg['num_frames']} bf16_x3tail/throughput tail={tail}: vs oracle " +
          " / ".join(f"{e:.2e}" for e in errs) + " | bf16 yardstick " + " / ".join(f"{e:.2e}" for e in yard))
    for e, yd in zip(errs, yard):
        assert np.isfinite(e) and e < 2.0 * yd + 2e-3, (label, case.over, errs, yard)
    return errs, yard


def _rows(case, label, engine="throughput", **attrs):
    """tests/fuzz_cases.py part (2): the first two loop iterations in the plain-bf16 phase, sample b of the batch against the same sample drawn
    alone (same Philox key, sample_offset = b): bit-identical where both runs are the small-batch engine's, <= 5e-5 on the throughput kernels."""
    model, diffusion = case.build("bf16_x3tail" + ("/throughput" if engine == "throughput" else ""), x3_tail=case.S - 2, **attrs)
    if engine != "throughput":
        eng, _ = model._get_engine(case.B, case.cfg["num_frames"])
        assert "sb_gemm" in eng.plan_query(case.B, case.guided) and "sb_gemm" in eng.plan_query(1, case.guided), "both runs must be the small-batch engine's"
    full = case.sample(model, diffusion, seed=7)
    dev = 0.0
    for b in sorted({0, case.B - 1}):
        yb = {k: v[b:b + 1] for k, v in case.y.items()}
        one = case.sample(model, diffusion, y=yb, shape=(1,) + case.shape[1:], seed=7, sample_offset=b)
        dev = max(dev, float((full[b:b + 1] - one).abs().max()))
    _close(model)
    print(f"\n[geometry] {label} {_tag(case.over)} B={case.B} T={case.cfg['num_frames']} {engine}: row consistency {dev:.1e}")
    assert bool(torch.isfinite(full).all())
    assert dev == 0.0 if engine != "throughput" else dev < ROW_TOL, (label, case.over, engine, dev)
    return dev


# ---- 1. head count on the fused in_proj + attention kernel (direct-to-LDS k_qkv_attn: every width but 512) -----------------------------
@pytest.mark.parametrize("T,B", [(16, 3), (64, 3), ("grid", "grid")])
@pytest.mark.parametrize("over", gc.HEADS_FUSED, ids=_tag)
def test_head_counts_on_the_fused_in_proj_attention_kernel(over, T, B):
    """k_qkv_attn<x3> and k_qkv_attn<plain> at H = 1, 2, 8 (it only ever ran at d = 512, H = 4, where the register-streamed forms take over), one
    token tile and two full ones, a half-empty sample pair (B = 3: one head per workgroup), and the other branch of its grid rule
    `pairs * H <= 64 ? H : (H % 2 == 0 ? 2 : 1)`: H = 8, B = 18 - 9 pairs x 8 > 64, four heads back to back; H = 1, B = 130 at T = 8 - one head,
    65 pairs; H = 2, B = 66 - 33 pairs x 2 > 64."""
    H = over["num_heads"]
    if T == "grid":
        T, B = (8, 130) if H == 1 else ((16, 66) if H == 2 else (16, 18))
        assert (B + 1) // 2 * H > 64
    else:
        assert (B + 1) // 2 * H <= 64
    case = Case(dict(over, num_frames=T), B, seed=H)
    _x3(case, "heads/fused", want=["k_qkv_attn"], never=["k_attn_x3", "k_attention", "k_sb_gemm"])
    _sched(case, "heads/fused", 3, want_plain=["k_qkv_attn"], want_split=["k_qkv_attn"], never_plain=["k_attn_x3", "k_attention", "k_qkv_attn_rs"])
    _rows(case, "heads/fused")


# ---- 2. head dim classes at d = 512 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["throughput", "small-batch", "f32"])
@pytest.mark.parametrize("T", [60, 100])
@pytest.mark.parametrize("over", gc.HEADS_D512, ids=_tag)
def test_head_dim_classes_at_d512(over, T, engine):
    """k_attn_x3 at dh = 64, 32, 16: behind k_rowgemm's in_proj in the plain phase where dh % 32 == 0 (H = 8, 16), behind the generic GEMM
    otherwise (H = 32) and in the split phase; the small-batch engine (rgn_sb.hip) with dh != 128. precision f32 on the same cases: k_attn_mfma at
    those head dims (60 tokens: two key tiles, 28 live rows in the second; 100: four, 4 live rows in the last) under the parity bound."""
    H = over["num_heads"]
    case = Case(dict(over, num_frames=T), 3, seed=H)
    if engine == "f32":
        _f32(case, "heads/d512", want=["k_gemm_f32", "k_attn_mfma"], never=["k_attention", "k_attn_x3"])
        return
    if engine == "small-batch":
        _x3(case, "heads/d512", engine, want=["k_sb_gemm", "k_attn_x3"])
        _rows(case, "heads/d512", engine)
        return
    _x3(case, "heads/d512", want=["k_attn_x3", "k_gemm_x3", "k_mlp_x3"], never=["k_sb_gemm", "k_qkv_attn"])
    inproj = ["k_rowgemm<ACT>"] if (512 // H) % 32 == 0 else ["k_gemm_x3"]
    _sched(case, "heads/d512", 3, want_plain=["k_attn_x3", "k_mlp2"] + inproj, want_split=["k_attn_x3"],
           never_plain=["k_qkv_attn_rs", "k_qkv_attn_long", "k_attention"] + (["k_rowgemm<ACT>"] if H == 32 else []))
    _rows(case, "heads/d512")


def test_one_token_sequences_through_the_scattering_in_proj():
    """T = 1 with heads of 64: the in_proj GEMM that scatters q / k / v per (sample, head) divides the row index by Tq with a 32-bit magic
    number, which does not exist for Tq = 1 - only whole 128-row tiles take that path, so B = 130 (one whole tile, one edge tile)."""
    case = Case(dict(num_heads=8, num_frames=1), 130, seed=1)
    _x3(case, "heads/T=1", want=["k_gemm_x3", "k_attn_x3"], never=["k_qkv_attn", "k_sb_gemm"])
    _sched(case, "heads/T=1", 3, want_plain=["k_gemm_x3", "k_attn_x3"], never_plain=["k_rowgemm<ACT>", "k_step"])
    _rows(case, "heads/T=1")


# ---- 3. fp32 attention inside the bf16 modes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,etd", [(161, False), (200, False), (160, True)])
@pytest.mark.parametrize("over", gc.PLAIN_ATTN, ids=_tag)
def test_fp32_attention_inside_the_bf16_modes(over, T, etd):
    """Heads of 8 (d = 512 / H = 64, d = 64 / H = 8) and more than 160 tokens fall to AF_PLAIN: the generic in_proj GEMM + the fp32 k_attention,
    in both bf16 modes; the small-batch engine is off for such handles. precision f32 runs (and reports) the same k_attention there, never
    k_attn_mfma, whose tiles stop at 160 tokens and start at heads of 16."""
    case = Case(dict(over, num_frames=T, emb_trans_dec=etd), 3, seed=T)
    model, _ = case.build("bf16_x3tail")                               # (the default engine selection: no "/throughput")
    for split in (False, True):
        _check_plan(case.kernels(model, split), ["k_attention"], ["k_sb_gemm", "k_attn_x3"])
    _close(model)
    _x3(case, "attn/fp32", want=["k_attention"], never=["k_attn_x3", "k_sb_gemm", "k_qkv_attn"])
    _sched(case, "attn/fp32", 3, want_plain=["k_attention"], want_split=["k_attention"], never_plain=["k_attn_x3", "k_qkv_attn_long"])
    _rows(case, "attn/fp32")
    _f32(case, "attn/fp32", want=["k_gemm_f32", "k_attention"], never=["k_attn_mfma", "k_attn_x3"])


# ---- 4. FFN width ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over", gc.FF_WIDTHS, ids=_tag)
def test_ffn_widths_and_their_k_padding(over):
    """k_rowgemm at K = 384 (ff = 384: k_rowgemm<LN> + k_rowgemm<ACT> layer tail), hidden widths that are no multiple of 32 (ff = 100, 1000:
    the K-padding columns of the hidden-tensor planes are zeroed once and no epilogue may write them - two sampling calls per handle), widths
    on both sides of every instantiated depth; the small-batch engine at ff = 1056 and its refusal: ff % 32 != 0, and ff < 512 - its linear1 launch leaves the
    residual stream's columns to the workgroups of their column block, so at ff = 32, 96, 384 columns ff .. 511 stayed unwritten (measured 2.2 - 4.8
    against the oracle before sb_supported refused them); such handles run the throughput kernels."""
    ff, d = over["ff_size"], over.get("latent_dim", 512)
    case = Case(dict(over, num_frames=60), 3, seed=ff % 97)
    _x3(case, "ffn", want=["k_gemm_x3", "k_layernorm"], never=["k_mlp_x3", "k_sb_gemm"], calls=2)
    rowgemm = d == 512 and ff == 384
    _sched(case, "ffn", 3, calls=2, want_plain=["k_rowgemm<LN>", "k_rowgemm<ACT>", "k_qkv_attn_rs"] if rowgemm else ["k_gemm_x3", "k_layernorm"],
           never_plain=["k_mlp2"] + ([] if rowgemm else ["k_rowgemm<LN>", "k_step"]))
    _rows(case, "ffn")
    sb = d == 512 and ff % 32 == 0 and ff >= 512                         # sb_supported (rgn_sb.hip)
    if sb:
        _x3(case, "ffn", "small-batch", want=["k_sb_gemm"], calls=2)
        _rows(case, "ffn", "small-batch")
    else:   # refused: the default engine selection runs the throughput kernels for this handle, whatever the batch size
        _x3(case, "ffn", "default", want=["k_gemm_x3", "k_layernorm"], never=["k_sb_gemm"], calls=2)


# ---- 5. feature width at the fused step boundary ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("over", gc.F_STEP, ids=_tag)
def test_feature_widths_at_the_step_boundary_k_step(over):
    """k_step's F loop at full width (F = 352: no K padding at all) and at each remainder (324, 340, 348): the kernel-per-stage chain ending
    in k_step, five motions of 60 frames (300 rows: four full 64-row tiles and a part of one), DDPM and its noise."""
    case = Case(dict(over, num_frames=60), 5, sampler="ddpm", seed=over["njoints"])
    _sched(case, "F/k_step", 2, want_plain=["k_step", "k_qkv_attn_rs", "k_mlp2"], never_plain=["k_update"])
    _rows(case, "F/k_step")


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("over", gc.F_STEP, ids=_tag)
def test_feature_widths_at_the_step_boundary_k_layers_multi_step(over, guided):
    """... and the step boundary inside k_layers<true>: B = 64, T = 52, one layer, 4 steps (3 plain-bf16 in ONE launch + 1 split-bf16), unguided
    and guided (a motion per workgroup: k_layers<true, true>), on-device Philox noise - the oracle runs on the very draws, re-made through
    rgn_randn_step."""
    B, S, seed = 64, 4, 11
    case = Case(dict(over, num_frames=52), B, S=S, sampler="ddpm", guided=guided, seed=over["njoints"] + int(guided))
    out = {}
    for prec in ("bf16_x3tail/throughput", "bf16/throughput"):
        model, diffusion = case.build(prec, x3_tail=1 if "tail" in prec else None, f16_steps=0, layers_guided=2, layers_min_b=1)
        if "tail" in prec:
            _check_plan(case.kernels(model, False), ["k_layers<true, true>" if guided else "k_layers<true>"], ["k_step", "k_step<guided>", "k_update"])
            eng, _ = model._get_engine(B, 52)
            st, buf = torch.cuda.current_stream().cuda_stream, torch.empty(case.shape, device="cuda")
            tape = np.empty((S + 1,) + case.shape, dtype=np.float32)
            for k, loop_index in enumerate([-1] + list(range(S - 1, -1, -1))):     # draw order: x_T, then loop indices S-1 .. 0
                eng.randn_step(buf, B, seed, 0, loop_index, st)
                tape[k] = buf.cpu().numpy()
            ref = case.oracle(tape=tape)
            out[prec] = case.sample(model, diffusion, seed=seed).cpu().numpy()
            dev = 0.0
            for b in (0, B - 1):   # row consistency: the single motion runs the same one-kernel form (layers_min_b = 1)
                one = case.sample(model, diffusion, y={k: v[b:b + 1] for k, v in case.y.items()}, shape=(1,) + case.shape[1:], seed=seed, sample_offset=b)
                dev = max(dev, float(np.abs(out[prec][b:b + 1] - one.cpu().numpy()).max()))
        else:
            out[prec] = case.sample(model, diffusion, tape=tape).cpu().numpy()
        _close(model)
    err, yard = float(np.abs(out["bf16_x3tail/throughput"] - ref).max()), float(np.abs(out["bf16/throughput"] - ref).max())
    print(f"\n[geometry] F/k_layers<true> {_tag(over)} B={B} T=52 guided={int(guided)}: vs oracle {err:.2e} | bf16 yardstick {yard:.2e} | row consistency {dev:.1e}")
    assert np.isfinite(err) and err < 2.0 * yard + 2e-3, (over, guided, err, yard)
    assert dev < ROW_TOL, (over, guided, dev)


# ---- 6. feature width off the fused step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over", gc.F_OFF_STEP, ids=_tag)
def test_feature_widths_off_the_fused_step(over):
    """F = 320 and 356 (the K padding of the input embedding is not 352), 32, 33, 263 and 1: no k_step, no k_layers<true> - the unfused output
    projection, k_update and input embedding with F padded to 32."""
    case = Case(dict(over, num_frames=60), 3, sampler="ddpm", seed=over["njoints"])
    _x3(case, "F/unfused", never=["k_step", "k_layers<true>"], want=["k_update"])
    _sched(case, "F/unfused", 3, want_plain=["k_update", "k_qkv_attn_rs", "k_mlp2"], never_plain=["k_step", "k_layers<true>"])
    _rows(case, "F/unfused")
    model, _ = Case(dict(over, num_frames=60), 64).build("bf16_x3tail")       # (at the batch size where the preset takes the multi-step kernel)
    eng, _ = model._get_engine(64, 60)
    plan = eng.plan_query(64, False, split_phase=False)
    assert "steps_fused" not in plan and "step_fused" not in plan and "layers" in plan, plan
    _close(model)


# ---- 7. short sequences ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", gc.SHORT_T)
def test_short_sequences(T):
    """Tiles that hold many samples: 1, 2, 7, 8 tokens (k_rowgemm takes Tq >= 8), and the lengths on each side of mlp_supported
    (63 / Tq + 2 <= M2::NSAMP = 4: k_rowgemm<LN> at 21 tokens, k_mlp2 from 22) and of mlp_x3_supported (31 / Tq + 2 <= MX::NSAMP = 2:
    k_gemm_x3 + k_layernorm at 31, k_mlp_x3 from 32). B = 7: a 64-row tile of T = 1 holds all of them."""
    assert (gc.TQ_MLP, gc.TQ_MLP_X3) == (22, 32)
    case = Case(dict(num_frames=T, layers=2), 7, seed=T)
    _x3(case, "short", want=["k_mlp_x3"] if T >= gc.TQ_MLP_X3 else ["k_layernorm"], never=[] if T >= gc.TQ_MLP_X3 else ["k_mlp_x3"])
    tail = ["k_mlp2"] if T >= gc.TQ_MLP else (["k_rowgemm<LN>"] if T >= 8 else ["k_layernorm"])
    _sched(case, "short", 3, want_plain=tail, never_plain=[k for k in ("k_mlp2", "k_rowgemm<LN>") if k not in tail] + ([] if T >= 8 else ["k_step"]))
    _rows(case, "short")
    _x3(case, "short", "small-batch", want=["k_sb_gemm"])
    _rows(case, "short", "small-batch")


# ---- 8. conditioning widths -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over", gc.CONDITIONING, ids=_tag)
def test_conditioning_widths(over):
    """The embedding paths in front of the layers: a text projection of 100 and of 768 features (K padded to 128 / exactly 768), a single action
    class; guided, so the masked-condition rows run too."""
    case = Case(dict(over, num_frames=32), 3, guided=True, seed=over.get("clip_dim", 1) % 89)
    _x3(case, "cond", want=["k_qkv_attn_rs_x3", "k_mlp_x3"])
    _x3(case, "cond", "small-batch", want=["k_sb_gemm"])
    model, diffusion = case.build("f32")
    _check_plan(case.kernels(model, True), ["k_gemm_f32", "k_attn_mfma"])
    err = float(np.abs(case.sample(model, diffusion).cpu().numpy() - case.ref).max())
    _close(model)
    print(f"\n[geometry] cond {_tag(over)} f32: vs oracle {err:.2e}")
    assert err < BOUND, (over, err)
    _rows(case, "cond", "small-batch")


# ---- 9. depth -------------------------------------------------------------------------------------------------------------------------
def test_nine_layers_run_the_kernel_per_stage_chain():
    """L = 9 is one more than k_layers' layer table holds (LY_MAXL = 8): at B = 64, T = 60, where the preset takes the one-kernel stack, the plain
    phase runs k_qkv_attn_rs + k_mlp2 + k_step per layer / step instead."""
    case = Case(dict(layers=9, num_frames=60), 64, S=2, sampler="ddpm", seed=9)
    _sched(case, "depth", 1, want_plain=["k_qkv_attn_rs", "k_mlp2", "k_step"], never_plain=["k_layers<false>", "k_layers<true>"])
    _rows(case, "depth")
