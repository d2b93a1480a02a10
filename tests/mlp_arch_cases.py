"""What tests/golden/make_golden_mlp.py and the arch='mlp' tests share: the recorded cases and the rule that rebuilds their in-painting inputs."""
import numpy as np

from regennet_amd import synth

# name -> (config, B, timesteps, guided, timesteps also recorded with y['uncond'], also one call with a different timestep per sample)
# (the 150-frame shape is recorded in two files: a committed file stays below 1 MiB)
FORWARD = {
    "mlp_tiny_fwd": ("tiny_mlp", 3, [0, 500, 999], False, [500], True),          # T = 8: below one MFMA k-step
    "mlp_tiny_text_fwd": ("tiny_text_mlp", 2, [0, 10, 999], False, [], True),    # T = 11: odd
    "mlp_tiny_fwd_cfg": ("tiny_mlp", 3, [0, 700, 999], True, [], True),          # guided: e_l differs between the halves
    "mlp_ntu_fwd": ("ntu_mlp", 3, [0, 10, 999], False, [], True),                # T = 60, d = 512, L = 8
    "mlp_chi3d_fwd": ("chi3d_mlp", 2, [0, 999], False, [], False),         # T = 150: several k-steps and row tiles, padded to 160
    "mlp_chi3d_fwd_mid": ("chi3d_mlp", 2, [700], False, [], True),
}
# name -> (config, B, respacing, sampler, guided, in-painting)
LOOPS = {
    "mlp_tiny_add_ddpm10": ("tiny_add_mlp", 2, "10", "ddpm", False, False),
    "mlp_tiny_ddim10_cfg": ("tiny_mlp", 2, "ddim10", "ddim", True, False),
    "mlp_ntu_ddpm50": ("ntu_mlp", 2, "50", "ddpm", False, False),
    "mlp_chi3d_ddim20_cfg": ("chi3d_mlp", 1, "ddim20", "ddim", True, False),
    "mlp_tiny_inpaint_ddpm10": ("tiny_mlp", 2, "10", "ddpm", False, True),
}


def inpaint_inputs(cfg, B):
    """mask [B,J,F,T] bool (True: keep the target): the first half of the frames of every row, and the translation row throughout;
    target: 0.5 x the x_T entry of the noise tape of seed 12."""
    J, Fe, T = cfg["njoints"], cfg["nfeats"], cfg["num_frames"]
    mask = np.zeros((B, J, Fe, T), dtype=bool)
    mask[..., : T // 2] = True
    mask[:, J - 1] = True
    target = (0.5 * synth.make_noise_tape(cfg, B, 0, seed=12)[0]).astype(np.float32)
    return mask, target
