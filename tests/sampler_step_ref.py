"""What the sampler-step tests share and what needs no GPU: the schedules, the reference step (oracle.regennet_oracle.sampler_step: torch CPU
float32 on the tables of orc.make_schedule, which owe nothing to rgn_plan.cpp or GaussianDiffusion._engine_tables) and the element-wise bound

    |x' - ref| <= 2^-22 * A,   A = the sum of the absolute values of the terms of the line
    DDPM   x' = c1 x0 + c2 x + sig eps                      A = |c1 x0| + |c2 x| + |sig eps|
    DDIM   x' = ca x0 + cb (sr x - x0) / srm1 + sig eps     A = |ca x0| + |cb| (|sr x| + |x0|) / |srm1| + |sig eps|

Two float32 ulps of the largest term: every product, sum and quotient of the line is rounded once on either side and the same way, and the one
factor that is not (sig of DDPM = exp(logvar / 2): expf on the host that builds the engine's table, torch.exp in the reference) is a
last-place difference of the noise term. "The same way" needs correctly rounded operations on the host too: torch's CPU sqrt is not (a last
place off on up to a fifth of its arguments, by host), and ddim_sample's sqrt(1 - abp - sigma^2) cancels, so the oracle's step takes its square
roots correctly rounded (oracle.regennet_oracle._sqrt; profiles/sampler_stream_parity.txt has the figures from before). A wrong coefficient, an entry taken at a neighbouring index or another order of operations moves
the result by many times that (tests/test_noise_stream_cpu.py shows it for alphas_cumprod_prev)."""
import numpy as np
import torch

from oracle import regennet_oracle as orc

BOUND = 2.0 ** -22
# name -> (noise_schedule, timestep_respacing, sigma_small)
SCHEDULES = {
    "cosine1000": ("cosine", "", True),
    "linear1000": ("linear", "", True),
    "cosine_ddim5": ("cosine", "ddim5", True),
    "cosine8_large": ("cosine", "8", False),
}
SAMPLERS = {"ddpm": ("ddpm", 0.0), "ddim_eta0": ("ddim", 0.0), "ddim_eta0.5": ("ddim", 0.5), "ddim_eta1": ("ddim", 1.0)}


def schedule(name):
    noise_schedule, resp, sigma_small = SCHEDULES[name]
    return orc.make_schedule(noise_schedule, resp, sigma_small=sigma_small)


def loop_indices(S):
    """S - 1, S / 2, 2, 1, 0: the first step, the middle, the two where 1 - ab / abp cancels, and the nz = 0 line."""
    return sorted({S - 1, S // 2, 2, 1, 0}, reverse=True)


def step_ref(tb, i, x, x0, eps, mode, eta, clip):
    """(x', pred_xstart) of the reference at loop index i: float32 CPU tensors in, float32 CPU tensors out."""
    with torch.no_grad():
        return orc.sampler_step(tb, i, x, x0, eps, mode, eta, clip)


def terms(tb, i, x, x0, eps, mode, eta):
    """A (float64 numpy, the shape of x): x0 is the prediction AFTER the clamp. Coefficients from the float32 table entries, in float64."""
    f = lambda name: float(np.float32(tb[name][i]))
    x, x0, eps = (np.abs(np.asarray(v, dtype=np.float64)) for v in (x, x0, eps))
    nz = 0.0 if i == 0 else 1.0
    if mode == "ddpm":
        sig = nz * np.exp(0.5 * f("model_log_variance"))
        return abs(f("posterior_mean_coef1")) * x0 + abs(f("posterior_mean_coef2")) * x + sig * eps
    # sigma and cb as the line itself forms them, in float32: 1 - abp - sigma^2 cancels (eta = 1 at the first steps of the cosine schedule leaves
    # a few bits), and the terms of the line are the terms with the coefficient the line uses
    ab, abp, one = np.float32(f("alphas_cumprod")), np.float32(f("alphas_cumprod_prev")), np.float32(1)
    sigma = np.float32(eta) * np.sqrt((one - abp) / (one - ab)) * np.sqrt(one - ab / abp)
    cb = float(np.sqrt(one - abp - sigma * sigma))
    assert sigma.dtype == np.float32
    return float(np.sqrt(abp)) * x0 + cb * (f("sqrt_recip_alphas_cumprod") * x + x0) / abs(f("sqrt_recipm1_alphas_cumprod")) + nz * float(sigma) * eps


def prev_read_at_i(tb):
    """The WRONG table a planner would build that took alphas_cumprod_prev one index off (entry i of alphas_cumprod instead of entry i - 1)."""
    bad = dict(tb)
    bad["alphas_cumprod_prev"] = np.array(tb["alphas_cumprod"], copy=True)
    return bad


def prev_one_step_early(tb):
    """... and the other neighbour: entry i - 2 (1.0 in front)."""
    bad = dict(tb)
    bad["alphas_cumprod_prev"] = np.append(1.0, tb["alphas_cumprod_prev"][:-1])
    return bad
