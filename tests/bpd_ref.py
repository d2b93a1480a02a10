"""Restatement of the reference's likelihood evaluation (diffusion/gaussian_diffusion.py:228-287, :419-423, :1204-1237, :1528-1601 with
diffusion/losses.py:12-77) in torch, parametrised on dtype, written from the formulas of include/regennet_hip.h above rgn_vb_terms.
tests/test_bpd_cpu.py pins its fp64 run to values recorded from the reference; its fp32 run is the reference's arithmetic at the precision a
user runs it in, and |fp32 - fp64| is the yardstick `d` of the 4 d rule (tests/test_bpd_gpu.py).

Rows: N = n_t x B in (timestep, motion) order, row r of motion r % B. `coef` [N, 6] fp32 holds, per row, posterior_mean_coef1,
posterior_mean_coef2, posterior_log_variance_clipped, the model's log variance, sqrt_recip_alphas_cumprod and sqrt_recipm1_alphas_cumprod."""
import math

import numpy as np
import torch

TERMS = ("vb", "xstart_mse", "mse")
LOW, HIGH, MARGIN = -0.999, 0.999, 1e-4          # the branches of the discretised likelihood, and how far the constructed inputs stay from them


def coef_rows(diffusion, t):
    """[N, 6] fp32 for loop indices t [N]: the fp64 table entries rounded to fp32, as _extract_into_tensor(...).float() does."""
    t = np.asarray(t, dtype=np.int64)
    tabs = (diffusion.posterior_mean_coef1, diffusion.posterior_mean_coef2, diffusion.posterior_log_variance_clipped,
            diffusion._model_variance_tables()[1], diffusion.sqrt_recip_alphas_cumprod, diffusion.sqrt_recipm1_alphas_cumprod)
    return np.stack([tab[t] for tab in tabs], 1).astype(np.float32)


def q_coef_rows(diffusion, t):
    t = np.asarray(t, dtype=np.int64)
    return np.stack([diffusion.sqrt_alphas_cumprod[t], diffusion.sqrt_one_minus_alphas_cumprod[t]], 1).astype(np.float32)


def _rows(a, dtype, N):
    a = torch.as_tensor(np.asarray(a)).to(dtype)
    return a.reshape(a.shape[0], -1) if a.dim() > 1 else a


def q_sample_rows_ref(x_start, noise, qcoef):
    """fp32 [N, ...]: a_r * x_start[r % B] + s_r * noise_r, two products and an add."""
    x0, nz, qc = torch.as_tensor(x_start), torch.as_tensor(noise), torch.as_tensor(qcoef)
    N, B = nz.shape[0], x0.shape[0]
    x0 = x0.repeat((N // B,) + (1,) * (x0.dim() - 1))
    shape = (N,) + (1,) * (x0.dim() - 1)
    return (qc[:, 0].reshape(shape) * x0 + qc[:, 1].reshape(shape) * nz).numpy()


def approx_standard_normal_cdf(x):
    return 0.5 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3))))


def discretized_gaussian_log_likelihood(x, means, log_scales):
    centered_x = x - means
    inv_stdv = torch.exp(-log_scales)
    cdf_plus = approx_standard_normal_cdf(inv_stdv * (centered_x + 1.0 / 255.0))
    cdf_min = approx_standard_normal_cdf(inv_stdv * (centered_x - 1.0 / 255.0))
    log_cdf_plus = torch.log(cdf_plus.clamp(min=1e-12))
    log_one_minus_cdf_min = torch.log((1.0 - cdf_min).clamp(min=1e-12))
    cdf_delta = cdf_plus - cdf_min
    return torch.where(x < LOW, log_cdf_plus, torch.where(x > HIGH, log_one_minus_cdf_min, torch.log(cdf_delta.clamp(min=1e-12))))


def normal_kl(mean1, logvar1, mean2, logvar2):
    return 0.5 * (-1.0 + logvar2 - logvar1 + torch.exp(logvar1 - logvar2) + ((mean1 - mean2) ** 2) * torch.exp(-logvar2))


def vb_terms_ref(x_start, x_t, output, noise, t, coef, clip, dtype=torch.float64):
    """-> float64 [N, 3] (vb, xstart_mse, mse); noise None: the mse column is 0. Inputs are fp32 arrays; `dtype` is the arithmetic."""
    N = np.asarray(x_t).shape[0]
    x0 = _rows(x_start, dtype, N)
    B = x0.shape[0]
    x0 = x0.repeat(N // B, 1)
    xt, p = _rows(x_t, dtype, N), _rows(output, dtype, N)
    c = torch.as_tensor(np.asarray(coef, dtype=np.float32)).to(dtype)
    c1, c2, lv_q, lv_m, sr, srm1 = (c[:, k:k + 1].expand_as(xt) for k in range(6))
    if clip:
        p = p.clamp(-1, 1)
    mean_q = c1 * x0 + c2 * xt
    mean_m = c1 * p + c2 * xt
    kl = normal_kl(mean_q, lv_q, mean_m, lv_m).mean(1) / math.log(2.0)
    nll = (-discretized_gaussian_log_likelihood(x0, mean_m, 0.5 * lv_m)).mean(1) / math.log(2.0)
    vb = torch.where(torch.as_tensor(np.asarray(t)) == 0, nll, kl)
    xstart_mse = ((p - x0) ** 2).mean(1)
    if noise is None:
        mse = torch.zeros_like(vb)
    else:
        mse = (((sr * xt - p) / srm1 - _rows(noise, dtype, N)) ** 2).mean(1)
    return torch.stack([vb, xstart_mse, mse], 1).double().numpy()


def sens_rows(x_start, x_t, output, noise, t, coef, clip, step=1e-3, seed=17):
    """[N, 3]: per row and column the largest change of the fp64 restatement when `output` moves by +-step (1e-3: the project's documented
    output bound) - the maximum over the direction sign(output - x_start), its opposite and three random-sign draws, the recipe of `sens` in
    tests/golden/make_golden_bpd.py, for inputs no fixture recorded (another noise, hence another x_t)."""
    out = np.asarray(output, dtype=np.float64)
    N, B = out.shape[0], np.asarray(x_start).shape[0]
    base = vb_terms_ref(x_start, x_t, out, noise, t, coef, clip)
    toward = np.sign(out - np.tile(np.asarray(x_start, dtype=np.float64), (N // B,) + (1,) * (out.ndim - 1)))
    toward[toward == 0] = 1.0
    rng = np.random.Generator(np.random.PCG64(seed))
    sens = np.zeros_like(base)
    for sign in [toward, -toward] + [rng.choice([-1.0, 1.0], out.shape) for _ in range(3)]:
        sens = np.maximum(sens, np.abs(vb_terms_ref(x_start, x_t, out + step * sign, noise, t, coef, clip) - base))
    return sens


def prior_bpd_ref(diffusion, x_start, dtype=torch.float64):
    S = diffusion.num_timesteps
    x0 = _rows(x_start, dtype, None)
    a = torch.tensor(np.float32(diffusion.sqrt_alphas_cumprod[S - 1])).to(dtype)
    lv = torch.tensor(np.float32(diffusion.log_one_minus_alphas_cumprod[S - 1])).to(dtype).expand_as(x0)
    zero = torch.zeros((), dtype=dtype)
    return (normal_kl(a * x0, lv, zero, zero).mean(1) / math.log(2.0)).double().numpy()


# ---- constructed inputs -------------------------------------------------------------------------------------------------------------------
def make_inputs(B, N, shape, seed, out_scale=0.4):
    """x_start [B, *shape] with elements below -0.999, above 0.999 and between and none within MARGIN of either threshold (no branch of the
    discretised likelihood is decided by rounding); output [N, *shape] around x_start with elements outside [-1, 1]; noise [N, *shape]. fp32."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x0 = rng.uniform(-1.15, 1.15, (B,) + tuple(shape))
    for thr in (LOW, HIGH):
        near = np.abs(x0 - thr) < 10 * MARGIN
        x0[near] = thr + np.where(rng.random(int(near.sum())) < 0.5, -1.0, 1.0) * 20 * MARGIN
    x0 = x0.astype(np.float32)
    noise = rng.standard_normal((N,) + tuple(shape)).astype(np.float32)
    output = (np.tile(x0, (N // B,) + (1,) * len(shape)) + out_scale * rng.standard_normal((N,) + tuple(shape))).astype(np.float32)
    return x0, output, noise


def noise_tape(S, B, shape, seed):
    """[S, B, *shape] fp32 N(0, 1): entry k is the reference's k-th randn_like (timestep S - 1 - k). Fixtures store the seed."""
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((S, B) + tuple(shape)).astype(np.float32)


def inputs_are_decided(x0):
    lo, hi, mid = (x0 < LOW).any(), (x0 > HIGH).any(), ((x0 > LOW) & (x0 < HIGH)).any()
    return bool(lo and hi and mid and (np.abs(x0.astype(np.float64) - LOW) > MARGIN).all() and (np.abs(x0.astype(np.float64) - HIGH) > MARGIN).all())


def schedule(kind):
    """The three schedules of the kernel grid, as regennet_amd diffusions: 'cosine1000', 'cosine_r50', 'linear_large'."""
    from regennet_amd.diffusion import gaussian_diffusion as gd
    from regennet_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    name, resp, var = {"cosine1000": ("cosine", "", gd.ModelVarType.FIXED_SMALL), "cosine_r50": ("cosine", "50", gd.ModelVarType.FIXED_SMALL),
                       "linear_large": ("linear", "", gd.ModelVarType.FIXED_LARGE)}[kind]
    return SpacedDiffusion(use_timesteps=space_timesteps(1000, resp or [1000]), betas=gd.get_named_beta_schedule(name, 1000),
                           model_mean_type=gd.ModelMeanType.START_X, model_var_type=var, loss_type=gd.LossType.MSE)


# (label, schedule, B, n_t, shape, clip): rows in (t, b) order over the timesteps S - 1, 1 and 0 - a t == 0 row next to t != 0 rows in one call
GRID = [
    ("n105 cosine1000 B3 N9 clip", "cosine1000", 3, 3, (5, 3, 7), True),
    ("n105 linear_large B3 N9", "linear_large", 3, 3, (5, 3, 7), False),
    ("n240 cosine_r50 B3 N9 clip", "cosine_r50", 3, 3, (5, 6, 8), True),
    ("n240 cosine1000 B1 N1", "cosine1000", 1, 1, (5, 6, 8), False),
    ("n11088 cosine_r50 B2 N6", "cosine_r50", 2, 3, (56, 6, 33), False),
    ("n11088 linear_large B1 N3 clip", "linear_large", 1, 3, (56, 6, 33), True),
]


def grid_case(label):
    """-> dict(diffusion, B, N, t [N], x_start, x_t, output, noise, coef, clip) for a GRID row (n_t = 1: t = 0 alone)."""
    _, kind, B, n_t, shape, clip = next(g for g in GRID if g[0] == label)
    d = schedule(kind)
    S = d.num_timesteps
    ts = [S - 1, 1, 0][-n_t:] if n_t < 3 else [S - 1, 1, 0]
    t = np.repeat(np.array(ts), B)
    N = len(t)
    x0, output, noise = make_inputs(B, N, shape, seed=sum(map(ord, label)))
    x_t = q_sample_rows_ref(x0, noise, q_coef_rows(d, t))
    return dict(diffusion=d, B=B, N=N, t=t, x_start=x0, x_t=x_t, output=output, noise=noise, coef=coef_rows(d, t), clip=clip)
