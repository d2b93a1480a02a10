"""The in-painting fixtures' cases (tests/golden/inpaint_*.npz): one table, and the rule that rebuilds mask and target of a case, shared
by the recorder (tests/golden/make_golden_inpaint.py) and the tests. Nothing of a mask or a target is stored where it can be rebuilt:
the target is synth.make_noise_tape(cfg, B, 0, seed=12)[0] * target_scale, the mask follows the rule below, and a digest of both lies
beside the recorded result."""
import numpy as np

from regennet_amd import synth
from regennet_amd.sample.edit import in_between_mask, rows_mask

ROWS_B64 = [0, 1, 21, 42, 63]        # the samples of a B = 64 result that a fixture keeps
KEEP_ROWS = list(range(22)) + [55]   # pose rows the 'rows' masks keep (the CLI's --keep_rows 0-21,55)

# mask rule per sample: ("in_between", prefix_end, suffix_start) | ("rows", [row, ...]) | ("all", bool) | ("random", p, seed)
CASES = {
    "inpaint_tiny_ddpm10": dict(cfg_name="tiny", B=3, resp="10", mode="ddpm", guided=False, trace=True,
                                masks=[("in_between", 0.25, 0.75), ("all", False), ("all", True)]),
    "inpaint_tiny_ddim10_cfg": dict(cfg_name="tiny", B=2, resp="ddim10", mode="ddim", guided=True,
                                    masks=[("random", 0.5, 20), ("random", 0.5, 21)]),
    "inpaint_tiny_clip": dict(cfg_name="tiny", B=2, resp="10", mode="ddpm", guided=False, clip=True, target_scale=1.5,
                              masks=[("in_between", 0.25, 0.75)] * 2),
    "inpaint_ntu_ddpm50": dict(cfg_name="ntu", B=2, resp="50", mode="ddpm", guided=False,
                               masks=[("in_between", 0.25, 0.75), ("in_between", 0.1, 0.5)]),
    "inpaint_ntu_ddpm50_b64": dict(cfg_name="ntu", B=64, resp="50", mode="ddpm", guided=False, rows=ROWS_B64,
                                   masks=[("rows", KEEP_ROWS) if b % 2 == 0 else ("in_between", 0.25, 0.75) for b in range(64)]),
    "inpaint_ntu_action_ddim5_cfg_b64": dict(cfg_name="ntu_action", B=64, resp="ddim5", mode="ddim", guided=True, rows=ROWS_B64,
                                             masks=[("in_between", 0.25, 0.75)] * 64),
    "inpaint_chi3d_ddim20_cfg": dict(cfg_name="chi3d", B=1, resp="ddim20", mode="ddim", guided=True,
                                     masks=[("in_between", 0.25, 1.0)]),
    "inpaint_offline_ntu_ddpm50": dict(cfg_name="ntu_offline", B=2, resp="50", mode="ddpm", guided=False,
                                       masks=[("in_between", 0.25, 0.75)] * 2),
}


def sample_mask(shape1, rule):
    """bool [njoints, nfeats, T] of one sample: True = keep the target (gaussian_diffusion.py:323)."""
    kind = rule[0]
    if kind == "in_between":
        return in_between_mask((1,) + tuple(shape1), rule[1], rule[2])[0]
    if kind == "rows":
        return rows_mask((1,) + tuple(shape1), rule[1])[0]
    if kind == "all":
        return np.full(shape1, bool(rule[1]), dtype=bool)
    if kind == "random":
        return np.random.RandomState(int(rule[2])).rand(*shape1) < float(rule[1])
    raise ValueError(rule)


def case_inputs(name):
    """(case, cfg, mask bool [B,J,F,T], target fp32 [B,J,F,T]) of a fixture."""
    case = CASES[name]
    cfg = synth.get_config(case["cfg_name"])
    B = case["B"]
    shape1 = (cfg["njoints"], cfg["nfeats"], cfg["num_frames"])
    mask = np.stack([sample_mask(shape1, r) for r in case["masks"]])
    assert mask.shape == (B,) + shape1 and mask.dtype == bool
    target = (synth.make_noise_tape(cfg, B, 0, seed=12)[0] * np.float32(case.get("target_scale", 0.5))).astype(np.float32)
    return case, cfg, mask, target
