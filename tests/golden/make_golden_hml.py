"""Fixtures of the hml_vec post-processing, recorded by RUNNING THE REFERENCE (CPU, fp32) in the build container.

    python tests/golden/make_golden_hml.py

Each case stores the input in the model's layout (x [B, D, 1, T]), `mean`, `std`, and `expected` [B, J, 3, T]: what the reference's own fp32 run of
sample/cgenerate.py:149-152 returns - the permute, t2m_dataset.inv_transform (data_loaders/humanml/data/dataset.py:132: data * std + mean, stated
here on tensors because the dataset class needs the licensed files), the reference's recover_from_ric
(data_loaders/humanml/scripts/motion_process.py:415-430) and the closing view / permute. `ref64_gap` is, for orientation, the largest distance of
that run from the same call in fp64.

  hml_t196       B 1, D 263, T 196: the rotation velocities make |a| pass pi, so a wrong angle convention cannot hide
  hml_kit_t65    B 3, D 251
  hml_t1, hml_t2 B 2 each
  hml_raw_t64    B 2, statistics 0 / 1: the features as they are (the kernel runs it with NULL statistics)
  hml_masks      HML_ROOT_MASK, HML_LOWER_BODY_MASK, HML_UPPER_BODY_MASK and HML_JOINT_NAMES of the reference's data_loaders/humanml_utils.py

Only DATA is written: tests/golden/hml_*.npz."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
from tests import hml_ref  # noqa: E402

CASES = {"hml_t196": (1, 263, 196, 11, False), "hml_kit_t65": (3, 251, 65, 12, False), "hml_t1": (2, 263, 1, 13, False),
         "hml_t2": (2, 263, 2, 14, False), "hml_raw_t64": (2, 263, 64, 15, True)}


def reference_run(x, mean, std, dtype):
    from data_loaders.humanml.scripts.motion_process import recover_from_ric
    sample = torch.from_numpy(x).to(dtype)
    n_joints = 22 if sample.shape[1] == 263 else 21                                              # cgenerate.py:149
    sample = (sample.cpu().permute(0, 2, 3, 1) * torch.from_numpy(std).to(dtype) + torch.from_numpy(mean).to(dtype))      # :150, dataset.py:132
    sample = sample.float() if dtype == torch.float32 else sample
    sample = recover_from_ric(sample, n_joints)                                                  # :151
    return sample.view(-1, *sample.shape[2:]).permute(0, 2, 3, 1).contiguous().numpy()           # :152


def main():
    _ref_import.install()
    for name, (B, D, T, seed, raw) in CASES.items():
        x, mean, std = hml_ref.make_inputs(B, D, T, seed, raw)
        if raw:
            mean, std = np.zeros(D, np.float32), np.ones(D, np.float32)
        expected = reference_run(x, mean, std, torch.float32)
        assert expected.dtype == np.float32 and expected.shape == (B, hml_ref.joints_of(D), 3, T)
        # the same call in fp64 (torch.zeros(shape) in recover_root_rot_pos is fp32 by default: widened for this run only)
        torch.set_default_dtype(torch.float64)
        try:
            gap = float(np.abs(reference_run(x, mean, std, torch.float64) - expected).max())
        finally:
            torch.set_default_dtype(torch.float32)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, x=x, mean=mean, std=std, expected=expected, raw=np.array(raw), ref64_gap=np.array(gap))
        ang = np.cumsum(hml_ref.inv_transform(x, mean, std)[:, 0, :, 0], axis=1)
        print(f"{name}: x {x.shape} -> {expected.shape}  max|a| {np.abs(ang).max():.2f}  max|xyz| {np.abs(expected).max():.2f}  "
              f"fp32 run vs fp64 run {gap:.2e}  {os.path.getsize(path)} B")
    import data_loaders.humanml_utils as hu
    path = os.path.join(HERE, "hml_masks.npz")
    np.savez_compressed(path, HML_ROOT_MASK=hu.HML_ROOT_MASK, HML_LOWER_BODY_MASK=hu.HML_LOWER_BODY_MASK, HML_UPPER_BODY_MASK=hu.HML_UPPER_BODY_MASK,
                        HML_JOINT_NAMES=np.array(hu.HML_JOINT_NAMES))
    print(f"hml_masks: {hu.HML_ROOT_MASK.shape} x 3, {len(hu.HML_JOINT_NAMES)} names  {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
