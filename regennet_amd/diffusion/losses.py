"""KL divergence of two diagonal Gaussians and the mean over a sample's elements, as torch expressions: what `GaussianDiffusion._prior_bpd`
needs (one expression per call, no kernel). The per-row forms of the variational bound, the discretised decoder likelihood included, are
evaluated on the device by rgn_vb_terms (csrc/rgn_vb.hip); tests/bpd_ref.py restates all of them."""
import torch as th


def _as_tensor(value, like):
    return value if th.is_tensor(value) else th.as_tensor(value, dtype=like.dtype, device=like.device)


def normal_kl(mean1, logvar1, mean2, logvar2):
    """KL(N(mean1, exp(logvar1)) || N(mean2, exp(logvar2))) per element, in nats:
        0.5 (-1 + logvar2 - logvar1 + exp(logvar1 - logvar2) + (mean1 - mean2)^2 exp(-logvar2))
    summed left to right as written (the order the fp32 rounding of include/regennet_hip.h's formula refers to). Arguments broadcast; scalars
    take the dtype and device of the first tensor among them."""
    like = next((a for a in (mean1, logvar1, mean2, logvar2) if th.is_tensor(a)), None)
    if like is None:
        raise TypeError("normal_kl: one argument at least must be a tensor")
    lv1, lv2 = _as_tensor(logvar1, like), _as_tensor(logvar2, like)
    variance_part = -1.0 + lv2 - lv1 + th.exp(lv1 - lv2)
    return 0.5 * (variance_part + (mean1 - mean2) ** 2 * th.exp(-lv2))


def mean_flat(tensor):
    """[B, ...] -> [B]: the mean over everything but the batch axis."""
    return tensor.flatten(1).mean(dim=1) if tensor.dim() > 1 else tensor
