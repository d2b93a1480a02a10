"""Fixtures of the likelihood evaluation, recorded by RUNNING THE REFERENCE (CPU) in the build container.

    python tests/golden/make_golden_bpd.py

`GaussianDiffusion.calc_bpd_loop` and `_vb_terms_bpd` (diffusion/gaussian_diffusion.py:1546-1601, :1204-1237, with diffusion/losses.py) are run as
they stand, through `SpacedDiffusion` (diffusion/respace.py), with `randn_like` served from a seeded tape (_ref_import.NoiseTape).

  kernel cases      the "model" is a stub that returns a prescribed output and q_sample hands back a prescribed x_t (the fp32 q_sample of the
                    stored x_start and noise), so the terms depend on the stored tensors alone. Run in fp64. The reference's
                    `_extract_into_tensor` rounds every coefficient to fp32 and would leave the coefficient-only sub-expressions
                    (exp(logvar1 - logvar2), exp(-log_scales)) in fp32 arithmetic even then; for these runs its result is widened to fp64, so the
                    values are "fp64 arithmetic from fp32 inputs and fp32 coefficients", the convention of rgn_vb_terms.
  end-to-end cases  the reference's own CMDM(arch='online') on the synthetic checkpoint, fp32 as a user runs it; its x_t, mapped timesteps and
                    output are logged per timestep. The terms are then formed in fp64 from that recorded output, as in a kernel case. `sens`
                    is, per entry, the largest change when the recorded output moves by +-1e-3 (the project's documented output bound): the
                    maximum over the direction sign(output - x_start), its opposite and three random-sign draws.

Noise is stored as a PCG64 seed (tests/bpd_ref.py noise_tape), not as a tape. Only DATA is written: tests/golden/bpd_<case>.npz."""
import os
import sys
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
from regennet_amd import synth  # noqa: E402
from tests import bpd_ref  # noqa: E402

KEYS = ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")


def ref_diffusion(schedule="cosine", resp="", large=False):
    _ref_import.install()
    from diffusion import gaussian_diffusion as gd
    from diffusion.respace import SpacedDiffusion, space_timesteps
    return SpacedDiffusion(use_timesteps=space_timesteps(1000, resp or [1000]), betas=gd.get_named_beta_schedule(schedule, 1000, 1.0),
                           model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_LARGE if large else gd.ModelVarType.FIXED_SMALL,
                           loss_type=gd.LossType.MSE, rescale_timesteps=False, data_rep="rot6d", num_person=1, body_model="smplx")


def widened_coefficients():
    """The reference's _extract_into_tensor with its fp32 result widened to fp64 (see the module text)."""
    from diffusion import gaussian_diffusion as gd
    orig = gd._extract_into_tensor
    return mock.patch.object(gd, "_extract_into_tensor", lambda arr, t, shape: orig(arr, t, shape).double())


def ref_loop_f64(diffusion, x_start, x_t, output, noise, clip, y):
    """The reference's calc_bpd_loop in fp64 on prescribed tensors: x_t, output, noise [S, B, ...] in the loop's order (entry k = timestep
    S - 1 - k). -> its dict as float64 arrays."""
    S = diffusion.num_timesteps
    assert len(x_t) == len(output) == len(noise) == S
    calls = []

    def stub(x, ts, **kw):
        calls.append(ts.clone())
        return torch.from_numpy(np.asarray(output[len(calls) - 1])).double()

    diffusion.q_sample = lambda x_start, t, noise=None: torch.from_numpy(np.asarray(x_t[S - 1 - int(t[0])])).double()
    try:
        with widened_coefficients(), _ref_import.NoiseTape([np.asarray(n, dtype=np.float64) for n in noise]):
            out = diffusion.calc_bpd_loop(stub, torch.from_numpy(x_start).double(), clip_denoised=clip, model_kwargs={"y": y})
    finally:
        del diffusion.q_sample
    assert set(out) == set(KEYS) and all(v.dtype == torch.float64 for v in out.values()) and len(calls) == S
    return {k: v.numpy() for k, v in out.items()}


def rows_of(d, B):
    """[B, S] columns of the loop's dict -> [S * B, 3] rows in the loop's (t descending, b) order."""
    return np.stack([d[k].T.reshape(-1) for k in bpd_ref.TERMS], 1)


def kernel_cases():
    for name, (schedule, resp, large, B, shape, clip, seed) in {"k_n105_r4": ("cosine", "4", False, 3, (5, 3, 7), True, 1),
                                                                 "k_n240_large_r5": ("linear", "5", True, 2, (5, 6, 8), False, 2)}.items():
        d = ref_diffusion(schedule, resp, large)
        S = d.num_timesteps
        t = np.repeat(np.arange(S - 1, -1, -1), B)
        x0, output, noise = bpd_ref.make_inputs(B, S * B, shape, seed)
        assert bpd_ref.inputs_are_decided(x0)
        x_t = bpd_ref.q_sample_rows_ref(x0, noise, bpd_ref.q_coef_rows(d, t))
        with torch.no_grad():      # the reference's own q_sample in fp32 gives these very bits
            for k in range(S):
                tk = torch.full((B,), S - 1 - k, dtype=torch.long)
                assert torch.equal(d.q_sample(torch.from_numpy(x0), tk, torch.from_numpy(noise[k * B:(k + 1) * B])), torch.from_numpy(x_t[k * B:(k + 1) * B]))
        r = lambda a: a.reshape((S, B) + shape)      # noqa: E731
        out = ref_loop_f64(d, x0, r(x_t), r(output), r(noise), clip, {})
        # q_mean_variance / q_posterior_mean_variance at per-row differing t, widened coefficients, fp64
        tq = torch.from_numpy(np.array([S - 1, 1, 0][:B]))
        with widened_coefficients():
            qm = d.q_mean_variance(torch.from_numpy(x0).double(), tq)
            qp = d.q_posterior_mean_variance(torch.from_numpy(x0).double(), torch.from_numpy(x_t[:B]).double(), tq)
        path = os.path.join(HERE, f"bpd_{name}.npz")
        np.savez_compressed(path, schedule=np.array(schedule), resp=np.array(resp), large=np.array(large), B=np.array(B), clip=np.array(clip), t=t,
                            x_start=x0, x_t=x_t, output=output, noise=noise, expected=rows_of(out, B), tq=tq.numpy(),
                            q_mean=qm[0].numpy(), q_variance=qm[1][:, 0, 0, 0].numpy(), q_log_variance=qm[2][:, 0, 0, 0].numpy(),
                            qp_mean=qp[0].numpy(), qp_variance=qp[1][:, 0, 0, 0].numpy(), qp_log_variance=qp[2][:, 0, 0, 0].numpy(),
                            **{k: out[k] for k in KEYS})
        print(f"{name}: S {S}  vb[0] {out['vb'][0]}  prior {out['prior_bpd']}  {os.path.getsize(path)} B")
    # _vb_terms_bpd itself, rows of differing t in ONE call on the unrespaced schedule
    d, B, shape = ref_diffusion("cosine", ""), 2, (5, 3, 7)
    t = np.repeat(np.array([999, 1, 0]), B)
    x0, output, noise = bpd_ref.make_inputs(B, len(t), shape, 3)
    assert bpd_ref.inputs_are_decided(x0)
    x_t = bpd_ref.q_sample_rows_ref(x0, noise, bpd_ref.q_coef_rows(d, t))
    with widened_coefficients(), torch.no_grad():
        out = d._vb_terms_bpd(lambda x, ts, **kw: torch.from_numpy(output).double(), torch.from_numpy(np.tile(x0, (3, 1, 1, 1))).double(),
                              torch.from_numpy(x_t).double(), torch.from_numpy(t), clip_denoised=True, model_kwargs={"y": {}})
    assert torch.equal(out["pred_xstart"], torch.from_numpy(output).double().clamp(-1, 1))
    path = os.path.join(HERE, "bpd_k_rows_cos1000.npz")
    np.savez_compressed(path, schedule=np.array("cosine"), resp=np.array(""), large=np.array(False), B=np.array(B), clip=np.array(True), t=t, x_start=x0,
                        x_t=x_t, output=output, noise=noise, expected_vb=out["output"].numpy())
    print(f"k_rows_cos1000: vb {out['output'].numpy()}  {os.path.getsize(path)} B")


def e2e_cases():
    cases = {"e2e_tiny_r10": ("tiny", "10", 3, None), "e2e_tiny_cos1000": ("tiny", "", 3, [999, 998, 500, 2, 1, 0]), "e2e_ntu_action_r4": ("ntu_action", "4", 2, None)}
    for name, (cfg_name, resp, B, keep) in cases.items():
        cfg = synth.get_config(cfg_name)
        model, diffusion = _ref_import.build_reference(cfg, synth.make_state_dict(cfg, seed=0), resp)
        S = diffusion.num_timesteps
        shape = (cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
        x0 = synth.make_cmotion(cfg, B, seed=4)
        assert (np.abs(np.abs(x0.astype(np.float64)) - 0.999) > 1e-6).all()      # no branch of the decoder likelihood hangs on the dtype of the comparison
        tape = bpd_ref.noise_tape(S, B, shape, seed=23)
        y = {"cmotion": torch.from_numpy(synth.make_cmotion(cfg, B, seed=1))}
        if "action" in cfg["cond_mode"]:
            y["action"] = torch.from_numpy(synth.make_actions(cfg, B, seed=2))
        # the reference run as a user makes it: fp32, its own call chain; the wrapped model's call is logged
        log = []
        fwd = model.forward

        def logged(x, ts, **kw):
            out = fwd(x, ts, **kw)
            log.append((x.clone(), ts.clone(), out.clone()))
            return out

        model.forward = logged
        with _ref_import.NoiseTape(list(tape)), torch.no_grad():
            out32 = diffusion.calc_bpd_loop(model, torch.from_numpy(x0), clip_denoised=True, model_kwargs={"y": y})
        model.forward = fwd
        assert len(log) == S
        x_t = np.stack([c[0].numpy() for c in log])
        t_model = np.stack([c[1].numpy() for c in log])
        output = np.stack([c[2].numpy() for c in log])
        # the reference's x_t is the fp32 q_sample of x_start and the tape, bit for bit: tests rebuild it (bpd_ref.q_sample_rows_ref), none is stored
        t_loop = np.repeat(np.arange(S - 1, -1, -1), B)
        assert np.array_equal(x_t.reshape((S * B,) + shape), bpd_ref.q_sample_rows_ref(x0, tape.reshape((S * B,) + shape), bpd_ref.q_coef_rows(diffusion, t_loop)))
        out = ref_loop_f64(diffusion, x0, x_t, output, tape, True, y)
        rng = np.random.Generator(np.random.PCG64(17))
        toward = np.sign(output.astype(np.float64) - x0[None].astype(np.float64))
        toward[toward == 0] = 1.0
        sens = {k: np.zeros_like(out[k]) for k in bpd_ref.TERMS}
        for sign in [toward, -toward] + [rng.choice([-1.0, 1.0], output.shape) for _ in range(3)]:
            moved = ref_loop_f64(diffusion, x0, x_t, output.astype(np.float64) + 1e-3 * sign, tape, True, y)
            for k in bpd_ref.TERMS:
                sens[k] = np.maximum(sens[k], np.abs(moved[k] - out[k]))
        rel32 = max(float(np.abs(out32[k].double().numpy() - out[k]).max() / np.abs(out[k]).max()) for k in KEYS)
        cols = np.arange(S) if keep is None else np.array([S - 1 - t for t in keep])      # column k = timestep S - 1 - k
        path = os.path.join(HERE, f"bpd_{name}.npz")
        np.savez_compressed(path, cfg_name=np.array(cfg_name), over=np.array("{}"), resp=np.array(resp), B=np.array(B), tape_seed=np.array(23), cols=cols,
                            timesteps=S - 1 - cols, t_model=t_model[cols], model_output=output[cols], total_bpd=out["total_bpd"],
                            prior_bpd=out["prior_bpd"], **{k: out[k][:, cols] for k in bpd_ref.TERMS}, **{"sens_" + k: sens[k][:, cols] for k in bpd_ref.TERMS},
                            sens_total=sens["vb"].sum(1))
        print(f"{name}: S {S}  total_bpd {out['total_bpd']}  fp32 run vs fp64 terms, max rel {rel32:.2e}  max sens vb {sens['vb'].max():.2e} "
              f"xstart_mse {sens['xstart_mse'].max():.2e} mse {sens['mse'].max():.2e}  {os.path.getsize(path)} B")


if __name__ == "__main__":
    kernel_cases()
    e2e_cases()
