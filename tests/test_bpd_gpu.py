"""GPU: rgn_q_sample_rows and rgn_vb_terms (csrc/rgn_vb.hip), diffusion.calc_bpd_loop / _vb_terms_bpd and `eval.score --bpd` against the fp64
restatement that tests/test_bpd_cpu.py pins to the reference.

Bound, per row and column (the rule of tests/test_losses_gpu.py): the fp32 run of the SAME restatement deviates from its fp64 run by d - the
reference arithmetic at the precision a user runs it in, computed here on the same inputs, never taken from the kernel. The kernel must stay
within 4 d, with one fp32 spacing of the value as floor (its result is an fp32 number). REGENNET_BPD_TABLE=<file> writes the measured table
(profiles/bpd_parity.txt)."""
import os

import numpy as np
import pytest
import torch

from regennet_amd import _lib, synth
from tests import bpd_ref
from tests import philox_ref as P
from tests.bpd_ref import TERMS

pytestmark = pytest.mark.gpu
TABLE = []
E2E = ["bpd_e2e_tiny_r10", "bpd_e2e_tiny_cos1000", "bpd_e2e_ntu_action_r4"]


@pytest.fixture(scope="module")
def engine():
    """One tiny model on the GPU: its engine is the finalized handle every kernel call below runs on."""
    from tests.helpers import build_hip
    cfg = synth.get_config("tiny")
    model, _ = build_hip(cfg, synth.make_state_dict(cfg, seed=0), resp="5")
    eng, _ = model._get_engine(3, cfg["num_frames"])
    yield eng
    if TABLE and os.environ.get("REGENNET_BPD_TABLE"):
        with open(os.environ["REGENNET_BPD_TABLE"], "w") as f:
            f.write(f"rgn_vb_terms on {torch.cuda.get_device_name(0)}: |kernel - fp64 restatement| against the bound max(4 x |fp32 restatement - fp64 restatement|, "
                    "1 fp32 spacing), per case and column at the row with the largest error / bound\n")
            f.write(f"{'case':52s} {'column':10s} {'value':>11s} {'fp32 ref':>10s} {'bound':>10s} {'kernel':>10s}\n")
            for row in TABLE:
                f.write("%-52s %-10s %11.4e %10.3e %10.3e %10.3e\n" % row)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_vb(eng, x_start, x_t, output, noise, t, coef, clip):
    """Engine.vb_terms on numpy inputs -> numpy [N, 3] fp32."""
    out = torch.full((len(t), 3), float("nan"), device="cuda")
    eng.vb_terms(dev(x_start), dev(x_t), dev(output), dev(noise), dev(np.asarray(t, dtype=np.int32)), dev(coef), _lib.VB_CLIP if clip else 0, out,
                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_case(eng, c, noise=True, rows=None):
    rows = slice(None) if rows is None else rows
    return run_vb(eng, c["x_start"], c["x_t"][rows], c["output"][rows], c["noise"][rows] if noise else None, c["t"][rows], c["coef"][rows], c["clip"])


def restate(x_start, x_t, output, noise, t, coef, clip):
    return tuple(bpd_ref.vb_terms_ref(x_start, x_t, output, noise, t, coef, clip, dtype=dt) for dt in (torch.float64, torch.float32))


def check(label, got, r64, r32, columns=(0, 1, 2), extra=None, truth=None):
    """got [N, 3] within the 4 d rule of r64 (or, with `truth` and `extra` [N, 3], within extra + the rule's bound of `truth`)."""
    assert got.shape == r64.shape == r32.shape and got.dtype == np.float32 and np.isfinite(got).all() and np.isfinite(r64).all(), label
    truth = r64 if truth is None else truth
    failed = []
    for k in columns:
        worst = None
        for r in range(got.shape[0]):
            d = abs(r32[r, k] - r64[r, k])
            bound = max(4 * d, float(np.spacing(np.float32(abs(r64[r, k]))))) + (0.0 if extra is None else float(extra[r, k]))
            err = abs(float(got[r, k]) - truth[r, k])
            if err > bound:
                failed.append((TERMS[k], r, err, bound))
            if worst is None or err / bound > worst[0]:
                worst = (err / bound, abs(truth[r, k]), d, bound, err)
        TABLE.append((label, TERMS[k]) + worst[1:])
        print("%-52s %-10s value %.4e  fp32 ref %.3e  bound %.3e  kernel %.3e" % ((label, TERMS[k]) + worst[1:]))
    assert not failed, (label, failed)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- rgn_vb_terms -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bpd_k_n105_r4", "bpd_k_n240_large_r5", "bpd_k_rows_cos1000"])
def test_kernel_fixtures(engine, golden, name):
    from tests.test_bpd_cpu import fixture_diffusion
    g = golden(name)
    coef = bpd_ref.coef_rows(fixture_diffusion(g), g["t"])
    args = (g["x_start"], g["x_t"], g["output"], g["noise"], g["t"], coef, bool(g["clip"]))
    got = run_vb(engine, *args)
    r64, r32 = restate(*args)
    if "expected" in g:
        assert float((np.abs(r64 - g["expected"]) / np.abs(g["expected"])).max()) < 1e-12      # (the restatement is the recorded reference run)
        check(name, got, r64, r32, truth=g["expected"])
    else:
        truth = r64.copy()
        truth[:, 0] = g["expected_vb"]
        assert float((np.abs(r64[:, 0] - g["expected_vb"]) / np.abs(g["expected_vb"])).max()) < 1e-12
        check(name, got, r64, r32, truth=truth)


@pytest.mark.parametrize("label", [row[0] for row in bpd_ref.GRID])
def test_grid(engine, label):
    """Odd n below one wave's worth of float4s, the tiny config's n, n = 56 x 6 x 33 (many strides per thread); B = 1 with N = 1, rows in (t, b)
    order with t == 0 next to t != 0; three schedules; the clamp on and off with outputs outside [-1, 1]; and without noise: the mse column is 0,
    the others unchanged bit for bit."""
    c = bpd_ref.grid_case(label)
    got = run_case(engine, c)
    r64, r32 = restate(c["x_start"], c["x_t"], c["output"], c["noise"], c["t"], c["coef"], c["clip"])
    check(label, got, r64, r32)
    bare = run_case(engine, c, noise=False)
    assert np.array_equal(bits(bare[:, :2]), bits(got[:, :2])) and not bare[:, 2].any() and got[:, 2].all()
    if c["N"] > 1:      # the clamp is not a no-op on these inputs
        other = run_vb(engine, c["x_start"], c["x_t"], c["output"], c["noise"], c["t"], c["coef"], not c["clip"])
        assert not np.array_equal(bits(other[:, 1]), bits(got[:, 1]))


def test_rows_do_not_depend_on_the_call_and_runs_are_identical(engine):
    c = bpd_ref.grid_case("n105 cosine1000 B3 N9 clip")
    full, again = run_case(engine, c), run_case(engine, c)
    assert np.array_equal(bits(full), bits(again))
    for r in range(c["N"]):
        b = r % c["B"]
        one = run_vb(engine, c["x_start"][b:b + 1], c["x_t"][r:r + 1], c["output"][r:r + 1], c["noise"][r:r + 1], c["t"][r:r + 1], c["coef"][r:r + 1], c["clip"])
        assert np.array_equal(bits(one), bits(full[r:r + 1])), r


# ---- rgn_q_sample_rows --------------------------------------------------------------------------------------------------------------------------
def run_q(eng, x_start, noise, qcoef, t, seed=0, sample_offset=0, want_noise=False):
    N = len(t)
    x_t = torch.full((N,) + x_start.shape[1:], float("nan"), device="cuda")
    nz = torch.full_like(x_t, float("nan")) if want_noise else None
    eng.q_sample_rows(dev(x_start), dev(noise), dev(qcoef), dev(np.asarray(t, dtype=np.int32)), seed, sample_offset, x_t, nz, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return x_t, nz


@pytest.mark.parametrize("label", ["n105 cosine1000 B3 N9 clip", "n11088 cosine_r50 B2 N6", "n240 cosine1000 B1 N1"])
def test_q_sample_rows_on_given_noise_is_q_sample_bit_for_bit(engine, label):
    c = bpd_ref.grid_case(label)
    d, B, N = c["diffusion"], c["B"], c["N"]
    x_t, nz = run_q(engine, c["x_start"], c["noise"], bpd_ref.q_coef_rows(d, c["t"]), c["t"], want_noise=True)
    x0_rows = dev(c["x_start"]).repeat((N // B, 1, 1, 1))
    want = d.q_sample(x0_rows, dev(c["t"]), dev(c["noise"]))           # per-row differing t, torch on the device
    assert torch.equal(x_t, want) and torch.equal(nz, dev(c["noise"]))
    assert np.array_equal(x_t.cpu().numpy(), c["x_t"])                   # ... and the host's fp32 expression


def test_q_sample_rows_draws_the_noise_of_randn_step(engine):
    """The engine's model is the tiny one ([5, 6, 8]): rgn_randn_step draws for exactly that shape."""
    d = bpd_ref.schedule("cosine1000")
    B, shape, seed, off = 3, (5, 6, 8), 0x9E3779B97F4A7C15, 2 ** 32 - 2      # motion 2 is sample 2^32: the carry into the counter's fourth word
    ts = [999, 7, 0]
    t = np.repeat(np.array(ts), B)
    x0, _, _ = bpd_ref.make_inputs(B, len(t), shape, 5)
    qc = bpd_ref.q_coef_rows(d, t)
    x_t, nz = run_q(engine, x0, None, qc, t, seed, off, want_noise=True)
    st = torch.cuda.current_stream().cuda_stream
    for k, tk in enumerate(ts):
        ref = torch.empty((B,) + shape, device="cuda")
        engine.randn_step(ref, B, seed, off, tk, st)
        assert torch.equal(nz[k * B:(k + 1) * B], ref), tk
    assert np.array_equal(x_t.cpu().numpy(), bpd_ref.q_sample_rows_ref(x0, nz.cpu().numpy(), qc))
    # every element against the host statement of the stream (the rule of tests/test_noise_stream_gpu.py: 4 E, E the fp32 formula's own rounding)
    F, T = shape[0] * shape[1], shape[2]
    for k, tk in enumerate(ts):
        ref = P.batch_normals_f64(seed, off, tk, B, F, T)
        E = float(np.abs(P.batch_normals_f32(seed, off, tk, B, F, T) - ref).max())
        assert float(np.abs(nz[k * B:(k + 1) * B].cpu().numpy().reshape(B, F, T) - ref).max()) <= 4 * E
    # the same rows issued in two calls, and without asking for the noise
    a, _ = run_q(engine, x0, None, qc[:B], t[:B], seed, off)
    b, _ = run_q(engine, x0, None, qc[B:], t[B:], seed, off)
    assert torch.equal(torch.cat([a, b]), x_t)
    # a motion's draw follows sample_offset + b, not the row
    shifted, _ = run_q(engine, x0[1:], None, qc[:2], t[:2], seed, off + 1)
    assert torch.equal(shifted, x_t[1:3])


# ---- calc_bpd_loop ------------------------------------------------------------------------------------------------------------------------------
class _Spy:
    """Stands where DistributedDataParallel stands (`.module` and a call), and logs the call."""

    def __init__(self, module):
        self.module, self.calls = module, []

    def __call__(self, x, ts, **kw):
        out = self.module(x, ts, **kw)
        self.calls.append((x.clone(), ts.clone(), out.clone()))
        return out

    def rows(self):
        return tuple(torch.cat([c[i] for c in self.calls]) for i in range(3))


def e2e_setup(g, precision="f32"):
    from tests.helpers import build_hip, fixture_cfg
    cfg = fixture_cfg(g)
    model, diffusion = build_hip(cfg, synth.make_state_dict(cfg, seed=0), resp=str(g["resp"]), precision=precision)
    B, S = int(g["B"]), diffusion.num_timesteps
    shape = (cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    x0 = synth.make_cmotion(cfg, B, seed=4)
    y = {"cmotion": torch.from_numpy(synth.make_cmotion(cfg, B, seed=1)).cuda()}
    if "action" in cfg["cond_mode"]:
        y["action"] = torch.from_numpy(synth.make_actions(cfg, B, seed=2)).cuda()
    tape = bpd_ref.noise_tape(S, B, shape, int(g["tape_seed"]))
    return model, diffusion, x0, y, tape


def close(model):
    for e in model._engines.values():
        e.close()


def rows_of(out, cols=None):
    """The loop's [B, S] columns -> [len(cols) * B, 3] rows in (column, b) order."""
    a = np.stack([out[k].cpu().numpy() if torch.is_tensor(out[k]) else out[k] for k in TERMS], -1)      # [B, S, 3]
    a = a if cols is None else a[:, cols]
    return np.ascontiguousarray(a.transpose(1, 0, 2)).reshape(-1, 3)


@pytest.mark.parametrize("name", E2E)
def test_calc_bpd_loop_end_to_end(golden, name):
    """diffusion.calc_bpd_loop on the recorded inputs and tape: every forward saw the reference's x_t bit for bit and the mapped timesteps and
    answered within 1e-3 of the reference's output; the returned columns are the restatement's on the device's own output (4 d rule) and lie
    within the recorded sensitivity to that 1e-3 (+ the rule's bound) of the reference's terms; total_bpd is vb.sum(1) + prior_bpd exactly;
    _vb_terms_bpd on one timestep returns the loop's column."""
    g = golden(name)
    model, diffusion, x0, y, tape = e2e_setup(g)
    try:
        B, S = int(g["B"]), diffusion.num_timesteps
        spy = _Spy(model)
        out = diffusion.calc_bpd_loop(spy, torch.from_numpy(x0).cuda(), clip_denoised=True, model_kwargs={"y": y}, noise_tape=torch.from_numpy(tape))
        assert set(out) == {"total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"} and all(v.is_cuda and v.dtype == torch.float32 for v in out.values())
        assert all(tuple(out[k].shape) == (B, S) for k in TERMS) and tuple(out["total_bpd"].shape) == tuple(out["prior_bpd"].shape) == (B,)
        assert len(spy.calls) == -(-S // max(1, 256 // B))
        x_t, ts, dev_out = spy.rows()
        t_loop = np.repeat(np.arange(S - 1, -1, -1), B)
        noise_rows = tape.reshape((S * B,) + x0.shape[1:])
        assert np.array_equal(x_t.cpu().numpy(), bpd_ref.q_sample_rows_ref(x0, noise_rows, bpd_ref.q_coef_rows(diffusion, t_loop)))
        assert ts.dtype == torch.long and ts.cpu().tolist() == [diffusion.timestep_map[t] for t in t_loop]      # the denoiser sees ORIGINAL timesteps
        cols = g["cols"]
        rec = (cols[:, None] * B + np.arange(B)[None, :]).reshape(-1)              # the recorded rows of the loop
        assert ts.cpu().numpy()[rec].tolist() == g["t_model"].reshape(-1).tolist() and (S - 1 - cols).tolist() == g["timesteps"].tolist()
        err = float(np.abs(dev_out.cpu().numpy()[rec].astype(np.float64) - g["model_output"].reshape((-1,) + x0.shape[1:])).max())
        print(f"{name}: max |device model output - reference's| = {err:.3e}")
        assert err < 1e-3, err
        coef = bpd_ref.coef_rows(diffusion, t_loop)
        r64, r32 = restate(x0, x_t.cpu().numpy(), dev_out.cpu().numpy(), noise_rows, t_loop, coef, True)
        got = rows_of(out)
        check(name + " (device output)", got, r64, r32)
        check(name + " (reference terms)", got[rec], r64[rec], r32[rec], extra=rows_of({k: g["sens_" + k] for k in TERMS}), truth=rows_of({k: g[k] for k in TERMS}))
        assert torch.equal(out["total_bpd"], out["vb"].sum(dim=1) + out["prior_bpd"])
        p64, p32 = bpd_ref.prior_bpd_ref(diffusion, x0, torch.float64), bpd_ref.prior_bpd_ref(diffusion, x0, torch.float32)
        assert (np.abs(out["prior_bpd"].cpu().numpy() - g["prior_bpd"]) <= np.maximum(4 * np.abs(p32 - p64), np.spacing(np.float32(g["prior_bpd"])))).all()
        # the total: each column's share of the bound and of the sensitivity, summed (an fp32 sum of S columns adds S roundings of the total)
        tot_bound = (np.maximum(4 * np.abs(r32[:, 0] - r64[:, 0]), np.spacing(np.abs(r64[:, 0]).astype(np.float32))).reshape(S, B).sum(0) + g["sens_total"]
                     + S * np.spacing(np.float32(g["total_bpd"])))
        assert (np.abs(out["total_bpd"].cpu().numpy() - g["total_bpd"]) <= tot_bound).all(), (out["total_bpd"], g["total_bpd"], tot_bound)
        # _vb_terms_bpd on one timestep (the loop's x_t): the restatement on its own output, the clamped prediction, and - where the loop can be
        # run with one timestep per evaluation in a few calls - the loop's column bit for bit
        k = int(cols[len(cols) // 2])
        t_vec = torch.full((B,), S - 1 - k, device="cuda", dtype=torch.long)
        spy1 = _Spy(model)
        one = diffusion._vb_terms_bpd(spy1, torch.from_numpy(x0).cuda(), x_t[k * B:(k + 1) * B], t_vec, clip_denoised=True, model_kwargs={"y": y})
        assert set(one) == {"output", "pred_xstart"} and tuple(one["output"].shape) == (B,)
        (_, ts1, out1), = spy1.calls
        assert ts1.tolist() == ts[k * B:(k + 1) * B].tolist() and torch.equal(one["pred_xstart"], out1.clamp(-1, 1))
        q64, q32 = restate(x0, x_t[k * B:(k + 1) * B].cpu().numpy(), out1.cpu().numpy(), None, t_loop[k * B:(k + 1) * B], coef[k * B:(k + 1) * B], True)
        row = np.zeros((B, 3), np.float32)
        row[:, 0] = one["output"].cpu().numpy()
        check(name + " (_vb_terms_bpd)", row, q64, q32, columns=(0,))
        # ... and the loop's column: the two forwards differ in their batch (B rows against a whole evaluation), hence within the recorded
        # sensitivity to the output bound (+ the rule's bound) of one another
        loop_col, sens_col = np.zeros((B, 3)), np.zeros((B, 3))
        loop_col[:, 0], sens_col[:, 0] = out["vb"][:, k].cpu().numpy(), g["sens_vb"][:, len(cols) // 2]
        check(name + " (_vb_terms_bpd vs the loop's column)", row, q64, q32, columns=(0,), extra=sens_col, truth=loop_col)
        raw = diffusion._vb_terms_bpd(model, torch.from_numpy(x0).cuda(), x_t[k * B:(k + 1) * B], t_vec, clip_denoised=False, model_kwargs={"y": y})
        assert torch.equal(raw["pred_xstart"], out1)
        if S <= 10:
            per_t = diffusion.calc_bpd_loop(model, torch.from_numpy(x0).cuda(), clip_denoised=True, model_kwargs={"y": y}, noise_tape=torch.from_numpy(tape),
                                            max_rows_per_call=B)
            assert torch.equal(one["output"], per_t["vb"][:, k])
    finally:
        close(model)


def test_grouping_into_calls_changes_no_bit_on_the_pinned_engine_form(golden):
    """max_rows_per_call = B, 2 B and 256: x_t is bit-equal whatever the engine; the terms are bit-equal with the engine form pinned as
    tests/test_hip_parity.py pins it for sample_auto_regressive (uniform split-bf16 on the small-batch engine), and within the recorded
    sensitivity otherwise."""
    g = golden("bpd_e2e_tiny_r10")
    B = int(g["B"])
    sens = np.stack([g["sens_" + k] for k in TERMS])
    for precision, exact in (("bf16x3", True), ("f32", False)):
        model, diffusion, x0, y, tape = e2e_setup(g, precision)
        try:
            runs = []
            for rows in (B, 2 * B, 256):
                spy = _Spy(model)
                out = diffusion.calc_bpd_loop(spy, torch.from_numpy(x0).cuda(), model_kwargs={"y": y}, noise_tape=torch.from_numpy(tape), max_rows_per_call=rows)
                runs.append((spy.rows()[0], torch.stack([out[k] for k in TERMS]), len(spy.calls)))
            assert [r[2] for r in runs] == [10, 5, 1]
            for x_t, terms, _ in runs[1:]:
                assert torch.equal(x_t, runs[0][0])
                if exact:
                    assert torch.equal(terms, runs[0][1])
                else:
                    diff = (terms.double() - runs[0][1].double()).abs().cpu().numpy()
                    assert (diff <= sens).all(), float((diff / sens).max())
        finally:
            close(model)


def test_seeded_runs_and_sample_offset(golden):
    """Drawn noise, the route `eval.score --bpd` takes. Two equal calls are bit-equal; the three columns of a seeded call, mse included, are the
    restatement's on the logged output and on the noise rgn_randn_step gives for (seed, sample_offset + b, t); a sub-batch with its
    sample_offset (motions 1.. at offset 1, motions ..2 at offset 0: what another --batch_size makes of the same motions) sees the same x_t bit
    for bit and returns the full call's rows within the sensitivity of those rows to the 1e-3 output bound (+ the rule's bound); the grouping
    into calls changes no bit on the pinned engine form; seed None follows torch's generator; another seed is another noise."""
    g = golden("bpd_e2e_tiny_r10")
    model, diffusion, x0, y, _ = e2e_setup(g, "bf16x3")
    try:
        B, S = int(g["B"]), diffusion.num_timesteps
        x0d = torch.from_numpy(x0).cuda()

        def run(lo=0, hi=B, **kw):
            spy = _Spy(model)
            out = diffusion.calc_bpd_loop(spy, x0d[lo:hi], model_kwargs={"y": {k: v[lo:hi] for k, v in y.items()}}, **kw)
            x_t, _, dev_out = spy.rows()
            return x_t, dev_out, out

        x_a, o_a, out_a = run(seed=5)
        x_b, _, out_b = run(seed=5)
        assert torch.equal(x_a, x_b) and all(torch.equal(out_a[k], out_b[k]) for k in out_a)
        # the noise a seeded call stands for, from rgn_randn_step; x_t and all three columns against the restatement on it
        noise = torch.empty((S * B,) + x0.shape[1:], device="cuda")
        for k in range(S):
            model._engine.randn_step(noise[k * B:(k + 1) * B], B, 5, 0, S - 1 - k, torch.cuda.current_stream().cuda_stream)
        noise = noise.cpu().numpy()
        t_loop = np.repeat(np.arange(S - 1, -1, -1), B)
        coef = bpd_ref.coef_rows(diffusion, t_loop)
        assert np.array_equal(x_a.cpu().numpy(), bpd_ref.q_sample_rows_ref(x0, noise, bpd_ref.q_coef_rows(diffusion, t_loop)))
        args = (x0, x_a.cpu().numpy(), o_a.cpu().numpy(), noise, t_loop, coef, True)
        r64, r32 = restate(*args)
        full = rows_of(out_a)
        check("seeded call (device output, randn_step noise)", full, r64, r32)
        assert torch.equal(out_a["total_bpd"], out_a["vb"].sum(dim=1) + out_a["prior_bpd"])
        # sub-batches with their sample_offset: the same x_t, and the full call's rows within their sensitivity to the output bound
        sens = bpd_ref.sens_rows(*args)
        for lo, hi in ((1, B), (0, 2)):
            x_k, _, out_k = run(lo=lo, hi=hi, seed=5, sample_offset=lo)
            pick = lambda a: a.reshape((S, B) + a.shape[1:])[:, lo:hi].reshape((S * (hi - lo),) + a.shape[1:])      # noqa: E731
            assert torch.equal(x_k, pick(x_a))
            check(f"seeded call, motions {lo}..{hi - 1} alone", rows_of(out_k), pick(r64), pick(r32), extra=pick(sens), truth=pick(full).astype(np.float64))
            assert torch.equal(out_k["prior_bpd"], out_a["prior_bpd"][lo:hi])
        # grouping into calls: no bit changes on the pinned engine form
        x_c, _, out_c = run(seed=5, max_rows_per_call=B)
        assert torch.equal(x_c, x_a) and all(torch.equal(out_c[k], out_a[k]) for k in out_a)
        x_o, _, out_o = run(seed=6)
        assert not torch.equal(x_o, x_a) and not torch.equal(out_o["mse"], out_a["mse"])
        torch.manual_seed(3)
        x_g, _, out_g = run()
        torch.manual_seed(3)
        x_h, _, out_h = run()
        assert torch.equal(x_g, x_h) and torch.equal(out_g["vb"], out_h["vb"]) and not torch.equal(x_g, x_a)
    finally:
        close(model)


def test_under_the_guidance_wrapper(golden):
    """ClassifierFreeSampleModel around the model: the call runs, the denoiser's guided output is what the terms are formed from (restatement on
    the logged output), and at scale 1 - where the reference's combination u + 1 (c - u) is the conditional output - the columns are the
    unguided call's within the recorded sensitivity."""
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    g = golden("bpd_e2e_tiny_r10")
    model, diffusion, x0, y, tape = e2e_setup(g)
    try:
        B, S = int(g["B"]), diffusion.num_timesteps
        t_loop = np.repeat(np.arange(S - 1, -1, -1), B)
        coef = bpd_ref.coef_rows(diffusion, t_loop)
        noise_rows = tape.reshape((S * B,) + x0.shape[1:])
        kw = dict(clip_denoised=True, noise_tape=torch.from_numpy(tape))
        plain = diffusion.calc_bpd_loop(model, torch.from_numpy(x0).cuda(), model_kwargs={"y": y}, **kw)
        outs = {}
        for scale in (2.5, 1.0):
            spy = _Spy(ClassifierFreeSampleModel(model))
            out = diffusion.calc_bpd_loop(spy, torch.from_numpy(x0).cuda(), model_kwargs={"y": dict(y, scale=torch.full((B,), scale, device="cuda"))}, **kw)
            x_t, ts, dev_out = spy.rows()
            assert ts.cpu().tolist() == [diffusion.timestep_map[t] for t in t_loop]
            r64, r32 = restate(x0, x_t.cpu().numpy(), dev_out.cpu().numpy(), noise_rows, t_loop, coef, True)
            check(f"guided scale {scale} (device output)", rows_of(out), r64, r32)
            outs[scale] = (out, dev_out)
        sens = rows_of({k: g["sens_" + k] for k in TERMS})
        diff = np.abs(rows_of(outs[1.0][0]).astype(np.float64) - rows_of(plain))
        bound = sens + 4 * np.spacing(np.abs(rows_of(plain)))
        assert (diff <= bound).all(), float((diff / bound).max())
        assert not torch.equal(outs[2.5][1], outs[1.0][1])
    finally:
        close(model)


def test_score_cli_bpd_prints_its_table_and_writes_the_per_motion_values(tmp_path, capsys):
    from regennet_amd.eval import score
    path = score.main(["--synthetic", "--bpd", "--timestep_respacing", "10", "--num_samples", "4", "--batch_size", "3", "--t_grid", "3",
                       "--output_dir", str(tmp_path)])
    text = capsys.readouterr().out
    res = np.load(path, allow_pickle=True).item()
    assert set(res) == {"total_bpd", "prior_bpd", "vb", "xstart_mse", "mse", "timesteps", "lengths"} and res["timesteps"].tolist() == list(range(10))
    assert all(res[k].shape == (10, 4) and np.isfinite(res[k]).all() for k in TERMS) and res["lengths"].shape == (4,)
    assert all(res[k].shape == (4,) and np.isfinite(res[k]).all() for k in ("total_bpd", "prior_bpd"))
    assert np.allclose(res["vb"].astype(np.float64).sum(0) + res["prior_bpd"], res["total_bpd"], rtol=1e-5)
    grid = score.timestep_grid(10, 3)
    lines = [ln.split() for ln in text.splitlines() if len(ln.split()) == 4 and ln.split()[0] in ["t"] + [str(t) for t in grid]]
    assert lines[0] == ["t", "vb", "xstart_mse", "mse"] and [int(ln[0]) for ln in lines[1:]] == grid == [0, 4, 9]
    for ln in lines[1:]:
        for j, k in enumerate(TERMS):
            want = float(res[k][int(ln[0])].mean())
            assert abs(float(ln[1 + j]) - want) <= 1e-5 * abs(want), (ln, k)
    last = [ln.split() for ln in text.splitlines() if ln.startswith("prior_bpd")]
    assert len(last) == 1 and abs(float(last[0][3]) - float(res["total_bpd"].mean())) <= 1e-5 * abs(float(res["total_bpd"].mean()))
    assert res["vb"][0].mean() != res["vb"][9].mean()            # ascending t: row 0 is the decoder term
