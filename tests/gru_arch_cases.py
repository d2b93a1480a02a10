"""What tests/golden/make_golden_gru_arch.py and the arch='gru' tests share: the recorded cases and the rule that rebuilds their in-painting inputs."""
from tests.mlp_arch_cases import inpaint_inputs  # noqa: F401  (the same rule: first half of the frames and the translation row)

# name -> (config, B, timesteps, guided, timesteps also recorded with y['uncond'], also one call with a different timestep per sample, scan)
FORWARD = {
    "gru_arch_tiny_fwd": ("tiny_gru", 3, [0, 500, 999], False, [500], True, "batch"),              # B = 3: three scan steps, T = 8 sequences (half a group)
    "gru_arch_tiny_fwd_frames": ("tiny_gru", 3, [0, 500, 999], False, [500], True, "frames"),
    "gru_arch_tiny_fwd_cfg": ("tiny_gru", 5, [0, 700, 999], True, [], True, "batch"),              # guided: two segments of B = 5 steps, emb differs between them
    "gru_arch_tiny_fwd_cfg_frames": ("tiny_gru", 3, [0, 700, 999], True, [], True, "frames"),      # guided: 6 sequences in one segment
    "gru_arch_tiny_add_fwd": ("tiny_add_gru", 5, [0, 10, 999], False, [], True, "batch"),          # no condition
    "gru_arch_tiny_text_fwd": ("tiny_text_gru", 3, [0, 10, 999], False, [10], True, "batch"),      # T = 11: odd; text condition
    "gru_arch_ntu_fwd": ("ntu_gru", 3, [0, 999], False, [], True, "batch"),                        # T = 60 (four groups, the last one ragged), d = 512, L = 8
}
# name -> (config, B, respacing, sampler, guided, in-painting, scan)
LOOPS = {
    "gru_arch_tiny_add_ddpm10": ("tiny_add_gru", 4, "10", "ddpm", False, False, "batch"),
    "gru_arch_tiny_ddim10_cfg": ("tiny_gru", 3, "ddim10", "ddim", True, False, "batch"),
    "gru_arch_tiny_ddim10_cfg_frames": ("tiny_gru", 3, "ddim10", "ddim", True, False, "frames"),
    "gru_arch_tiny_inpaint_ddpm10": ("tiny_gru", 2, "10", "ddpm", False, True, "batch"),
    "gru_arch_tiny_add_ddpm10_frames": ("tiny_add_gru", 2, "10", "ddpm", False, False, "frames"),
}
